// gemm_lowp_plan.hpp -- host-side plans of the weight-only GEMM: packed dimensions, the per-family launch plans, and THE route
// decision (plan_gemm): which of the six kernel families serves a call, with which template specialisation and which grid.
// gemm_lowp_plan.hip defines them; gemm_lowp.hip (launch + entry points), moe.hip, decode_attn_block.hip and
// decode_mlp_block.hip use them.  Everything here is a pure function of (call description, CU count, the six family switches
// of include/dashinfer_hip.h): no HIP call except cached_num_cus(), no allocation.
#pragma once
#include <algorithm>

#include "device_utils.h"

namespace dihip {

struct GemvArgs;  // gemv_stream_kernel.hpp

// ---- packed dimensions ("dihip tile-major", gemm_lowp.hip) --------------------------------------------------------------
struct LowpDims {
  int KTILE, Kp, KT, Np, NTILES, G, Gp, group;
  int Gp_packed;  // (scale, zero) groups stored per column tile: the pack kernel sizes them for the W4 padding of K
  int ktpg;       // k-tiles per quantisation group (per-channel / W16: >= KT; groups smaller than a k-tile: 0)
};
inline int roundup(int v, int m) { return (v + m - 1) / m * m; }
inline LowpDims lowp_dims(int wbits, int N, int K, int group_size) {
  LowpDims d;
  d.KTILE = wbits == 4 ? 128 : wbits == 8 ? 64 : 32;
  d.Kp = roundup(K, d.KTILE);
  d.KT = d.Kp / d.KTILE;
  d.Np = roundup(N, 16);
  d.NTILES = d.Np / 16;
  d.group = group_size > 0 ? group_size : 0;
  d.G = d.group ? (K + d.group - 1) / d.group : 1;
  d.Gp = d.group ? std::max(d.G, (d.Kp + d.group - 1) / d.group) : 1;
  d.Gp_packed = d.group ? std::max(d.G, (roundup(K, 128) + d.group - 1) / d.group) : 1;
  d.ktpg = d.group ? d.group / d.KTILE : (1 << 28);
  return d;
}

// ---- per-family plans ---------------------------------------------------------------------------------------------------
constexpr int GEMV_STREAM_MAX_M = 4;  // largest batch of the LDS-resident decode GEMV (beyond it the per-workgroup x staging,
                                      // M x K into LDS, costs more than the small-batch kernels)
constexpr size_t GEMM_SYNC_BYTES = 64 * 1024;  // up to 16384 (column-block x m-block) counters

struct GemmPlan {  // gemm_lowp_kernel.hpp
  int MT, NT, NTW, col_blocks, m_blocks, splitk, ktiles_per_split, kslice_tiles;
  size_t lds_bytes, slab_bytes;
};
struct GemvPlan {  // gemv_stream_kernel.hpp
  bool ok;
  int MR, upb, blocks, WK, WN, ktpg, kgroups, RS;
  size_t lds_bytes;
};
struct PanelPlan {  // gemm_panel_kernel.hpp
  bool ok;
  int panels, nslices, ktps;
  size_t slab_bytes;
};
struct KslicePlan {  // gemm_kslice_kernel.hpp
  bool ok;
  int groups, nslices, waves, nunits;
  size_t slab_bytes;
};
struct PrefillTail {  // gemm_prefill_kernel.hpp, PrefillArgs::tail_cb
  int col_blocks, mblocks, tail_cb, ksplit;
  size_t slab_bytes;
};
struct GembPlan {  // gemv_batch_kernel.hpp
  int upb, blocks;
};

GemmPlan make_plan(int wbits, int M, int N, int K, int group_size, bool dual);
// want_blocks > 0 (expert slots: gridDim.y multiplies the grid): aim at that many workgroups instead of one per CU
GemvPlan make_gemv_plan(int wbits, int M, int N, int K, int group_size, bool dual, int want_blocks = 0);
PrefillTail prefill_tail_plan(int wbits, int M, int N, int K, int group_size, bool dual);
// The plan fields of a decode GEMV's arguments -- the ONLY place they are written: the stand-alone launch, the expert slots
// (moe.hip) and the launches that run the GEMV's body inside another kernel (decode_attn_block.hip, decode_mlp_block.hip)
// are bit-identical to each other because they share it.  `blocks` workgroups own the NTILES column tiles.
void fill_gemv_plan(GemvArgs* g, const GemvPlan& p, const LowpDims& d, int blocks);
// The largest split-K slab a kernel family may ask for when it serves this shape (workspace sizing).
size_t lowp_slab_bytes(int wbits, int M, int N, int K, int group_size, bool dual);

// ---- the route ----------------------------------------------------------------------------------------------------------
enum GemmFamily { FAM_NONE = 0, FAM_GEMV_STREAM, FAM_GEMM_KSLICE, FAM_GEMM_PANEL, FAM_GEMV_BATCH, FAM_GEMM_PREFILL, FAM_GEMM_LOWP };

// One call of the weight-only GEMM as the C entry points hand it to run_gemm (gemm_lowp.hip).
struct GemmCall {
  int wbits, dtype, pro, epi;
  const void* x;
  int ldx;
  const void* gamma;
  float eps;
  const void *w0, *sz0, *w1, *sz1;
  const void *bias, *residual;
  void* y;
  const float* h_res;
  float* h_out;
  int M, N, K, group_size, act;
  float alpha;
  void* ws;
  size_t ws_bytes;
  void* sync;
  int x_layout, y_layout;  // DIHIP_ACT_ROWMAJOR / DIHIP_ACT_FRAG32 (small-batch kernels only)
  // EPI_ADDTO: RMSNorm of the finished rows wanted in n_out (dihip_fused_gemm_addto_norm); *n_done is set when the kernel
  // family that served the call has produced it (split-K slab reduction), otherwise the caller runs the norm kernel
  const void* n_gamma;
  float n_eps;
  void* n_out;
  int n_frag_mt;
  bool* n_done;
  // deferred RMSNorm (gemv_batch_kernel.hpp, GembArgs).  Producer: n_rowsq != null asks for n_out = FT(gamma * h_out) and the
  // row partials instead of the finished norm; *n_parts = parts written, 0 when the serving kernel does not offer it (the
  // norm is then produced as above).  Consumer: rowsq != null -- rows are scaled by 1 / rms on the accumulator.
  float* n_rowsq;
  size_t n_rowsq_bytes;
  int* n_parts;
  const float* rowsq;
  int rowsq_parts;
  float rowsq_eps;
};

// Everything the route depends on.  describe() fills it from a real call; the shape-only queries
// (dihip_gemm_lowp_prefers_frag, dihip_prenorm_rowsq_supported, the FRAG32 precondition of the entry points) use
// GemmDesc::of_shape(): 16-byte aligned pointers, ldx = K, an ample workspace and a sync buffer.
struct GemmDesc {
  int wbits, dtype, pro, epi, M, N, K, group_size;
  int x_layout, y_layout;  // DIHIP_ACT_ROWMAJOR / DIHIP_ACT_FRAG32
  int ldx;
  bool x_aligned, gamma_aligned, ws_aligned;  // 16 bytes
  size_t ws_bytes;                            // 0: no workspace
  bool has_sync, has_w1;
  bool rowsq;      // deferred row norms handed in (consumer)
  bool n_gamma;    // EPI_ADDTO: the RMSNorm of the finished rows is wanted as well
  size_t n_rowsq_bytes;  // ... deferred (producer) into a row-partial buffer of this size; 0: finished norm only
  static GemmDesc of_shape(int wbits, int dtype, int pro, int epi, int M, int N, int K, int group_size, int x_layout,
                           int y_layout);
};

struct GemmRoute {
  int family;          // FAM_NONE: not served -- `status` / `error` say why (need_bytes: the workspace that was missing)
  int status;
  const char* error;
  size_t need_bytes;
  // template key of the launch thunk: <wbits, dtype, mt (gemv_stream: MR), nt, pro, epi, gpt, rs>
  int mt, nt, pro, epi, gpt;
  int rs;              // gemm_kslice: the deferred-row-norm consumer instantiation
  unsigned grid[3];
  int threads;
  size_t lds_bytes;    // dynamic LDS
  size_t slab_bytes;   // split-K slab at the start of the workspace
  int ncu;             // CU count the plan was made for
  bool norm_in_reduce; // EPI_ADDTO + n_gamma: the norm rides on the slab reduction
  int prenorm_parts;   // gemv_batch producer of deferred row norms: parts written (0: not offered)
  // the family's plan
  GemvPlan gemv;
  KslicePlan kslice;
  PanelPlan panel;
  GembPlan gemb;
  PrefillTail prefill;  // ksplit == 1: unsplit grid
  GemmPlan gemm;
};

GemmDesc describe(const GemmCall& c);
GemmRoute plan_gemm(const GemmDesc& c);
// a PRO_PLAIN row-major call of this shape runs on the small-batch kernel, which reads FRAG32 activations faster
bool lowp_prefers_frag(int wbits, int M, int N, int K, int group_size, bool dual);
// a PRO_PLAIN call of this shape with FRAG32 activations in and out is served (by one of the small-batch kernels)
bool lowp_frag_served(int wbits, int dtype, int M, int N, int K, int group_size, bool dual);

// ---- decode GEMVs run from other translation units --------------------------------------------------------------------------
// One launch of M = 1 GEMVs over (token, expert-rank) slots (mixture-of-experts, moe.hip): slot s streams expert
// slot_expert[s] of a stack of equally shaped packed weights, reads activation row s / x_div, writes row s.
int run_gemv_slots(hipStream_t stream, int wbits, int epi, const void* x, int ldx, int x_div, const void* w0, const void* sz0,
                   const void* w1, const void* sz1, void* y, int N, int K, int group_size, const int* slot_expert, int nslots,
                   const int* group_rows, const int* group_nrows);
// One launch of the context-phase GEMM over the expert-sorted row tiles of a prompt (mixture-of-experts, moe.hip:
// gemm_prefill_kernel<.., GROUPED>): tile t = {expert, first sorted position, rows <= 128} of `tiles`, its rows are the slots
// sorted_slot[first ..], slot s reads activation row s / x_div and writes row s.  The grid is max_tiles x column blocks;
// workgroups past *ntiles (device memory) exit.  bf16, STD / SwiGLU, no tail split.
int run_prefill_grouped(hipStream_t stream, int wbits, int epi, const void* x, int ldx, int x_div, const void* w0, const void* sz0,
                        const void* w1, const void* sz1, void* y, int N, int K, int group_size, const int* tiles, const int* ntiles,
                        const int* sorted_slot, int max_tiles);
int prefill_grouped_col_blocks(int N, bool dual);  // column blocks of such a launch (dual: SwiGLU, 128 output columns each)
// The decode GEMV's plan for ONE row as the workgroups of ANOTHER launch run it (decode_attn_block.hip): the K split (WK, kcut)
// and the wave grid are those of the stand-alone launch -- the sums are then bit-identical to it -- while the column tiles are dealt
// over `nblocks` workgroups (block b owns tiles b, b + nblocks, ...).  Fills the shape / plan fields of *g (pointers are the
// caller's); *max_units = most tiles one workgroup owns, *lds_bytes = its LDS need.  False: shape not served by the decode GEMV.
bool gemv_block_plan(int wbits, int N, int K, int group_size, int nblocks, GemvArgs* g, int* max_units, size_t* lds_bytes);
// The stand-alone decode GEMV's plan and shape fields for one row, as run_gemm fills them (decode_mlp_block.hip runs the bodies of
// two such launches inside one: same blocks, same K split, same sums).  Pointers are the caller's.
bool gemv_plan_args(int wbits, int N, int K, int group_size, bool dual, GemvArgs* g, int* blocks, size_t* lds_bytes);

}  // namespace dihip
