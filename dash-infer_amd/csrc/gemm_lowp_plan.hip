// gemm_lowp_plan.hip -- the launch plans of the weight-only GEMM and its route decision (gemm_lowp_plan.hpp), plus the C
// entry points that answer from shapes alone.  Host code only: nothing here launches a kernel.
#include <cstdlib>

#include "gemm_lowp_plan.hpp"
#include "gemm_lowp_kernel.hpp"
#include "gemv_stream_kernel.hpp"
#include "gemm_prefill_kernel.hpp"
#include "gemv_batch_kernel.hpp"
#include "gemm_kslice_kernel.hpp"
#include "gemm_panel_kernel.hpp"

namespace dihip {

static int num_cus() {  // without a device: the MI355X's
  const int n = cached_num_cus();
  return n > 0 ? n : 256;
}

// ---- general kernel (gemm_lowp_kernel.hpp) ------------------------------------------------------------------------------
GemmPlan make_plan(int wbits, int M, int N, int K, int group_size, bool dual) {
  const LowpDims d = lowp_dims(wbits, N, K, group_size);
  GemmPlan p;
  p.MT = M > 16 ? 2 : 1;
  const int rows_per_block = 16 * p.MT;
  p.m_blocks = (M + rows_per_block - 1) / rows_per_block;
  const int target_blocks = (num_cus() * 5) / 2;
  // tiles per wave: 4 streams/wave normally; 2 when the matrix is too narrow to fill the chip
  p.NT = 4;
  if (!dual && wbits != 16) {
    const int cb4 = (d.NTILES + GEMM_WAVES * 4 - 1) / (GEMM_WAVES * 4);
    if ((long)cb4 * p.m_blocks * d.KT < target_blocks) p.NT = 2;
  }
  p.NTW = dual ? p.NT / 2 : p.NT;
  p.col_blocks = (d.NTILES + GEMM_WAVES * p.NTW - 1) / (GEMM_WAVES * p.NTW);
  // split-K granule: whole quantisation groups, whole k-tiles
  int granule = 1;
  if (d.group > d.KTILE) granule = (d.group + d.KTILE - 1) / d.KTILE;
  const int units = (d.KT + granule - 1) / granule;
  int want = (int)std::max<long>(1, target_blocks / std::max<long>(1, (long)p.col_blocks * p.m_blocks));
  want = std::min(want, units);
  // a skinny unquantised matrix (the MoE router, hidden -> 64 experts; the shared expert's gate, hidden -> 1) is ONE column block:
  // its last-arriving workgroup sums every split's partial tile alone -- 112 splits of one k-tile took 19.8 us (profiles/r03u),
  // most of it that serial sum
  if (wbits == 16 && (long)p.col_blocks * p.m_blocks <= 2) want = std::min(want, 16);
  int units_per_split = (units + want - 1) / want;
  p.ktiles_per_split = units_per_split * granule;
  p.splitk = (d.KT + p.ktiles_per_split - 1) / p.ktiles_per_split;
  // the activation slice is staged in LDS in pieces of at most ~60 KiB:
  // (rows+1) * (kslice*KTILE + 8) * 2 bytes
  const int rows = std::min(M, rows_per_block);
  const int max_tiles = std::max(1, (60 * 1024 / ((rows + 1) * 2) - 8) / d.KTILE);
  // several slices: each a multiple of the register ring depth (gemm_lowp_kernel.hpp)
  p.kslice_tiles = p.ktiles_per_split <= max_tiles ? p.ktiles_per_split : std::max(GEMM_RING, max_tiles / GEMM_RING * GEMM_RING);
  p.lds_bytes = GEMM_LDS_HEADER + (size_t)(rows + 1) * (p.kslice_tiles * d.KTILE + 8) * 2;
  p.slab_bytes = p.splitk > 1 ? (size_t)p.splitk * M * (dual ? 2 : 1) * d.Np * sizeof(float) : 0;
  return p;
}

// ---- decode fast path (gemv_stream_kernel.hpp) --------------------------------------------------------------------------
GemvPlan make_gemv_plan(int wbits, int M, int N, int K, int group_size, bool dual, int want_blocks) {
  GemvPlan p{};
  const LowpDims d = lowp_dims(wbits, N, K, group_size);
  p.ok = false;
  if (M < 1 || M > GEMV_STREAM_MAX_M) return p;
  if (d.group && d.group % d.KTILE != 0) return p;  // groups smaller than a k-tile: general kernel
  p.ktpg = d.ktpg;
  p.MR = M == 1 ? 1 : 4;
  p.RS = d.Kp + 8;
  const int ncu = num_cus();
  const int units = d.NTILES;
  // never more workgroups than CUs (a second round starts ~2 us late, measured on the qkv shape):
  // one tile per workgroup up to the CU count, ceil(tiles / CUs) beyond
  p.upb = units <= ncu ? 1 : (units + ncu - 1) / ncu;
  if (want_blocks > 0) p.upb = std::max(1, (units + want_blocks - 1) / want_blocks);
  p.blocks = (units + p.upb - 1) / p.upb;
  const int nv = p.upb * (dual ? 2 : 1);
  const int kgroups = d.group ? (d.KT + p.ktpg - 1) / p.ktpg : d.KT;
  // wave grid WK x WN: minimise the longest per-wave chunk sequence (ties: fewer k-slices)
  long best = -1;
  p.kgroups = kgroups;
  for (int wn = GEMV_WAVES; wn >= (dual ? 2 : 1); wn /= 2) {
    const int wkk = GEMV_WAVES / wn;
    if (wkk > kgroups) continue;
    const long load = (long)((nv + wn - 1) / wn) * ((kgroups + wkk - 1) / wkk);
    if (best < 0 || load < best) {
      best = load;
      p.WN = wn;
      p.WK = wkk;
    }
  }
  if (best < 0) {
    p.WN = GEMV_WAVES;
    p.WK = 1;
  }
  p.lds_bytes = gemv_lds_bytes(M, p.RS, d.KT, p.upb, dual, p.WK);
  if (p.lds_bytes > 150 * 1024) return p;
  p.ok = true;
  return p;
}

void fill_gemv_plan(GemvArgs* g, const GemvPlan& p, const LowpDims& d, int blocks) {
  g->KT = d.KT;
  g->NTILES = d.NTILES;
  g->Gp = d.Gp_packed;
  g->ktpg = p.ktpg;
  g->kgroups = p.kgroups;
  g->upb = p.upb;
  g->nu_q = d.NTILES / blocks;
  g->nu_r = d.NTILES % blocks;
  g->WK = p.WK;
  g->WN = p.WN;
  g->RS = p.RS;
  // K-slice boundaries in split units: the even split; wave w runs k-slice w % WK of column slot w / WK
  g->wmap = 0;
  for (int i = 0; i <= GEMV_WAVES; ++i) g->kcut[i] = i < p.WK ? (int)((long)p.kgroups * i / p.WK) : p.kgroups;
}

// shape fields of a one-row decode GEMV that another launch runs (pointers are the caller's)
static void fill_gemv_row(GemvArgs* g, int N, int K) {
  g->M = 1;
  g->N = N;
  g->K = K;
  g->ldx = K;
  g->ldy = N;
  g->alpha = 1.f;
  g->act = DIHIP_ACT_NONE;
}

bool gemv_block_plan(int wbits, int N, int K, int group_size, int nblocks, GemvArgs* g, int* max_units, size_t* lds_bytes) {
  const GemvPlan gp = make_gemv_plan(wbits, 1, N, K, group_size, false);
  const LowpDims d = lowp_dims(wbits, N, K, group_size);
  if (!gp.ok || gp.MR != 1 || K != d.Kp || nblocks < 1 || nblocks > d.NTILES) return false;
  fill_gemv_row(g, N, K);
  fill_gemv_plan(g, gp, d, nblocks);
  g->upb = g->nu_q + (g->nu_r ? 1 : 0);
  *max_units = g->upb;
  *lds_bytes = gemv_lds_bytes(1, gp.RS, d.KT, g->upb, 0, gp.WK);
  return true;
}

bool gemv_plan_args(int wbits, int N, int K, int group_size, bool dual, GemvArgs* g, int* blocks, size_t* lds_bytes) {
  const GemvPlan gp = make_gemv_plan(wbits, 1, N, K, group_size, dual);
  const LowpDims d = lowp_dims(wbits, N, K, group_size);
  if (!gp.ok || gp.MR != 1 || K != d.Kp) return false;
  fill_gemv_row(g, N, K);
  fill_gemv_plan(g, gp, d, gp.blocks);
  *blocks = gp.blocks;
  *lds_bytes = gp.lds_bytes;
  return true;
}

// ---- batched decode, FRAG32 activations (gemm_panel_kernel.hpp) ---------------------------------------------------------
static PanelPlan make_panel_plan(int wbits, int M, int N, int K, int group_size, bool dual) {
  PanelPlan p{};
  static const bool enabled = !env_off("DIHIP_GEMM_PANEL");  // =0: keep the whole-column kernel (diagnostics)
  if (!enabled) return p;
  const LowpDims d = lowp_dims(wbits, N, K, group_size);
  const int ncu = num_cus();
  p.panels = (d.NTILES + PANEL_WAVES - 1) / PANEL_WAVES;
  const int ktpg = d.group ? std::max(1, d.group / d.KTILE) : 1;  // slices hold whole quantisation groups
  if (2 * p.panels >= ncu) {
    p.nslices = 1;  // enough panels to keep the HBM queue full from every second CU on
    p.ktps = d.KT;
  } else {
    // few columns: split K so that about one workgroup lands on every CU, but keep >= 8 k-tiles per slice
    int s = std::max(1, ncu / p.panels);
    int ktps = (d.KT + s - 1) / s;
    ktps = (ktps + ktpg - 1) / ktpg * ktpg;
    if (ktps < 8) return p;  // the ring would never fill: the whole-column kernel handles these
    p.ktps = ktps;
    p.nslices = (d.KT + ktps - 1) / ktps;
  }
  p.slab_bytes = p.nslices > 1 ? (size_t)p.nslices * (dual ? 2 : 1) * M * N * sizeof(float) : 0;
  p.ok = true;
  return p;
}

// ---- batched decode, FRAG32 activations, register-resident K-slices (gemm_kslice_kernel.hpp) ----------------------------
static KslicePlan make_kslice_plan(int wbits, int M, int N, int K, int group_size, bool dual, bool sizing = false) {
  KslicePlan p{};
  // DIHIP_GEMM_KSLICE: 0 = never, 2 = every eligible shape (tests / diagnostics); read per call so that one process can
  // exercise both kernels
  const char* e = getenv("DIHIP_GEMM_KSLICE");
  const int mode = sizing ? 2 : e ? atoi(e) : 1;  // workspace sizing covers the forced mode as well
  if (mode == 0 || (wbits != 4 && wbits != 8)) return p;
  const LowpDims d = lowp_dims(wbits, N, K, group_size);
  const int ch = wbits == 4 ? 4 : 8;  // k-tiles per K-slice (16 k-steps of 32)
  if (d.KT % ch) return p;            // slices hold whole k-tiles of equal count
  if (wbits == 8 && d.group == d.KTILE) return p;  // W8 g64 (a scale per k-tile in a 16-slot ring) does not fit the register file
  // Measured against the panel kernel (tools/gemv_bench and bench.py, 7B and 72B/TP8 shapes): +13 % on the SwiGLU pair
  // at M = 16 (8 KiB in flight per wave), +4 % (gate/up) and +8 % (down, split-K slab) at M = 32, but 30-40 % slower on
  // matrices of a few MB (one or two half-units per workgroup: the ring never reaches steady state)
  if (mode != 2 && (size_t)N * K * wbits / 8 * (dual ? 2 : 1) < ((size_t)24 << 20)) return p;
  const int nsl = d.KT / ch;
  p.waves = std::min(KSL_WAVES, nsl);
  p.nslices = (nsl + KSL_WAVES - 1) / KSL_WAVES;
  p.nunits = d.NTILES;
  p.groups = std::max(1, std::min(p.nunits, num_cus() / p.nslices));  // one 8-wave workgroup per CU (64 KB LDS, ~250 registers)
  p.slab_bytes = p.nslices > 1 ? (size_t)p.nslices * (dual ? 2 : 1) * M * N * sizeof(float) : 0;
  p.ok = true;
  return p;
}

// ---- context phase (gemm_prefill_kernel.hpp) ----------------------------------------------------------------------------
// Tail split (PrefillArgs::tail_cb): when the grid of 128 x 256 tiles ends in a round that fills at most half the chip, the
// column blocks of that round are split in K instead -- `ksplit` workgroups per tile, whole quantisation groups each, all of
// them within one round -- and a reduction launch adds the parts.  Qwen2-7B at 2048 rows: qkv 288 tiles -> 256 + 32 x 7 parts
// (176 -> ~115 us), gate / up 2368 -> 2304 + 64 x 4.  DIHIP_PREFILL_TAIL_SPLIT=0: off.
PrefillTail prefill_tail_plan(int wbits, int M, int N, int K, int group_size, bool dual) {
  PrefillTail t{};
  const LowpDims d = lowp_dims(wbits, N, K, group_size);
  const int tpb = dual ? PF_WN * PF_CW / 2 : PF_WN * PF_CW;
  t.col_blocks = (d.NTILES + tpb - 1) / tpb;
  t.mblocks = (M + PF_BM - 1) / PF_BM;
  t.tail_cb = t.col_blocks;
  t.ksplit = 1;
  static const bool on = !env_off("DIHIP_PREFILL_TAIL_SPLIT");
  const int ncu = num_cus();
  const int blocks = t.col_blocks * t.mblocks, rem = blocks % ncu;
  if (!on || M < 64 || (wbits != 4 && wbits != 8) || blocks <= ncu || rem == 0 || rem > ncu / 2) return t;
  const int tcb = (rem + t.mblocks - 1) / t.mblocks, tiles = tcb * t.mblocks;
  if (tiles > ncu / 2 || tcb >= t.col_blocks) return t;
  const int ktpg = d.group ? d.group / d.KTILE : d.KT;
  const int units = d.group ? d.KT / std::max(ktpg, 1) : d.KT;  // K parts hold whole groups (per-channel: whole k-tiles)
  int best = 1;
  for (int ks = 2; ks <= 8; ++ks)
    if (units % ks == 0 && tiles * ks <= ncu) best = ks;
  if (best == 1) return t;
  t.tail_cb = t.col_blocks - tcb;
  t.ksplit = best;
  t.slab_bytes = (size_t)tiles * best * PF_BM * 256 * sizeof(float);
  return t;
}

size_t lowp_slab_bytes(int wbits, int M, int N, int K, int group_size, bool dual) {
  size_t slab = make_plan(wbits, M, N, K, group_size, dual).slab_bytes;
  if (wbits != 16 && M >= 64) slab = std::max(slab, prefill_tail_plan(wbits, M, N, K, group_size, dual).slab_bytes);
  if (wbits != 16 && M > GEMV_STREAM_MAX_M && M <= 32) {
    slab = std::max(slab, make_panel_plan(wbits, M, N, K, group_size, dual).slab_bytes);
    slab = std::max(slab, make_kslice_plan(wbits, M, N, K, group_size, dual, true).slab_bytes);
  }
  return slab;
}

// ---- the route ----------------------------------------------------------------------------------------------------------
static bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

GemmDesc describe(const GemmCall& c) {
  GemmDesc d{};
  d.wbits = c.wbits, d.dtype = c.dtype, d.pro = c.pro, d.epi = c.epi;
  d.M = c.M, d.N = c.N, d.K = c.K, d.group_size = c.group_size;
  d.x_layout = c.x_layout, d.y_layout = c.y_layout;
  d.ldx = c.ldx;
  d.x_aligned = aligned16(c.x), d.gamma_aligned = aligned16(c.gamma), d.ws_aligned = aligned16(c.ws);
  d.ws_bytes = c.ws ? c.ws_bytes : 0;
  d.has_sync = c.sync != nullptr;
  d.has_w1 = c.w1 && c.sz1;
  d.rowsq = c.rowsq != nullptr;
  d.n_gamma = c.n_gamma && c.n_out;
  d.n_rowsq_bytes = (d.n_gamma && c.n_rowsq && c.n_parts) ? c.n_rowsq_bytes : 0;
  return d;
}

GemmDesc GemmDesc::of_shape(int wbits, int dtype, int pro, int epi, int M, int N, int K, int group_size, int x_layout,
                            int y_layout) {
  GemmDesc d{};
  d.wbits = wbits, d.dtype = dtype, d.pro = pro, d.epi = epi;
  d.M = M, d.N = N, d.K = K, d.group_size = group_size;
  d.x_layout = x_layout, d.y_layout = y_layout;
  d.ldx = K;
  d.x_aligned = d.gamma_aligned = d.ws_aligned = true;
  d.ws_bytes = ~(size_t)0;
  d.has_sync = d.has_w1 = true;
  return d;
}

static GemmRoute not_served(GemmRoute r, int status, const char* error, size_t need_bytes = 0) {
  r.family = FAM_NONE;
  r.status = status;
  r.error = error;
  r.need_bytes = need_bytes;
  return r;
}
static void set_launch(GemmRoute& r, int family, unsigned gx, unsigned gy, unsigned gz, int threads, size_t lds_bytes,
                       size_t slab_bytes) {
  r.family = family;
  r.grid[0] = gx, r.grid[1] = gy, r.grid[2] = gz;
  r.threads = threads;
  r.lds_bytes = lds_bytes;
  r.slab_bytes = slab_bytes;
}

// The families in the order they are tried; the first that serves the call takes it.  The caller has validated the call
// (run_gemm: shape, dtype, group size, pointers).
GemmRoute plan_gemm(const GemmDesc& c) {
  GemmRoute r{};
  r.status = DIHIP_SUCCESS;
  r.ncu = num_cus();
  r.pro = c.pro;
  r.epi = c.epi;
  const bool dual = c.epi == EPI_SWIGLU;
  const LowpDims d = lowp_dims(c.wbits, c.N, c.K, c.group_size);
  const bool whole_groups = d.group == 0 || d.group % d.KTILE == 0;  // no group smaller than a k-tile
  const bool aligned = c.K == d.Kp && c.ldx % 8 == 0 && c.x_aligned && (c.pro == PRO_PLAIN || c.gamma_aligned);
  const bool want_frag = c.x_layout == DIHIP_ACT_FRAG32 || c.y_layout == DIHIP_ACT_FRAG32;  // small-batch kernels only
  const bool small_batch = c.M > GEMV_STREAM_MAX_M && c.M <= 32;
  static const bool decode_on = !env_off("DIHIP_GEMV_STREAM");  // =0 routes everything to the general kernel
  r.gpt = c.wbits != 16 && d.group == d.KTILE;                  // every k-tile is one quantisation group
  r.mt = c.M > 16 ? 2 : 1;
  if (c.rowsq && !(small_batch && c.dtype == DIHIP_BF16 && c.epi != EPI_ADDTO))
    return not_served(r, DIHIP_PARAM_ERROR,
                      "gemm_lowp: deferred row norms are taken by the small-batch kernels only (4 < M <= 32, bf16); see "
                      "dihip_prenorm_rowsq_supported");
  // the norm of the finished rows can ride on a split-K slab reduction (gemm_reduce_addto_norm_kernel)
  const bool norm_ridable = c.epi == EPI_ADDTO && c.n_gamma && c.N % 4 == 0 && c.N <= 8192;

  // batch 1 .. 4, row-major: activations resident in LDS (gemv_stream_kernel.hpp)
  if (decode_on && aligned && !want_frag) {
    r.gemv = make_gemv_plan(c.wbits, c.M, c.N, c.K, c.group_size, dual);
    if (r.gemv.ok) {
      r.mt = r.gemv.MR;
      set_launch(r, FAM_GEMV_STREAM, r.gemv.blocks, 1, 1, GEMV_THREADS, r.gemv.lds_bytes, 0);
      return r;
    }
  }
  // batched decode with FRAG32 activations: register-resident K-slices (gemm_kslice_kernel.hpp), else panels of 8 column
  // tiles sharing x through LDS (gemm_panel_kernel.hpp)
  if (decode_on && c.x_layout == DIHIP_ACT_FRAG32 && c.pro == PRO_PLAIN && small_batch && c.wbits != 16 && c.K == d.Kp &&
      whole_groups) {
    r.kslice = make_kslice_plan(c.wbits, c.M, c.N, c.K, c.group_size, dual);
    if (r.kslice.ok) {
      if (c.ws_bytes < r.kslice.slab_bytes)
        return not_served(r, DIHIP_MEMORY_ERROR, "gemm_kslice: workspace too small for the split-K slab", r.kslice.slab_bytes);
      r.rs = c.rowsq && r.kslice.nslices == 1;  // otherwise the slab reduction applies 1 / rms
      r.norm_in_reduce = norm_ridable && r.kslice.nslices > 1;
      set_launch(r, FAM_GEMM_KSLICE, r.kslice.groups, r.kslice.nslices, 1, r.kslice.waves * 64, 0, r.kslice.slab_bytes);
      return r;
    }
    r.panel = make_panel_plan(c.wbits, c.M, c.N, c.K, c.group_size, dual);
    if (r.panel.ok) {
      if (c.ws_bytes < r.panel.slab_bytes)
        return not_served(r, DIHIP_MEMORY_ERROR, "gemm_panel: workspace too small for the split-K slab", r.panel.slab_bytes);
      if (c.rowsq && r.panel.nslices == 1)
        return not_served(r, DIHIP_PARAM_ERROR,
                          "gemm_panel: deferred row norms need the split-K reduction; see dihip_prenorm_rowsq_supported");
      r.norm_in_reduce = norm_ridable && r.panel.nslices > 1;
      set_launch(r, FAM_GEMM_PANEL, r.panel.panels, r.panel.nslices, 1, PANEL_THREADS, 0, r.panel.slab_bytes);
      return r;
    }
  }
  // small decode batches whose activations do not fit in LDS: register-resident A (gemv_batch_kernel.hpp)
  if (decode_on && aligned && c.pro == PRO_PLAIN && c.M > 1 && c.M <= 32 && c.wbits != 16 && whole_groups) {
    if (c.rowsq && c.epi != EPI_STD)
      return not_served(r, DIHIP_PARAM_ERROR,
                        "gemv_batch: deferred row norms on the plain epilogue only; see dihip_prenorm_rowsq_supported");
    // at most one workgroup per CU; a workgroup with several units walks them two at a time so that
    // one pass over the activations (L2 -> registers) feeds two column tiles
    r.gemb.upb = d.NTILES <= r.ncu ? 1 : (d.NTILES + r.ncu - 1) / r.ncu;
    r.gemb.blocks = (d.NTILES + r.gemb.upb - 1) / r.gemb.upb;
    r.nt = r.gemb.upb >= 2 ? 2 : 1;
    if (c.epi == EPI_ADDTO && c.dtype == DIHIP_BF16 && r.gemb.upb <= GEMB_MAXU &&
        (size_t)r.gemb.blocks * 32 * sizeof(float) <= c.n_rowsq_bytes)  // deferred RMSNorm, producer side
      r.prenorm_parts = r.gemb.blocks;
    set_launch(r, FAM_GEMV_BATCH, r.gemb.blocks, 1, 1, GEMB_THREADS, 0, 0);
    return r;
  }
  if (want_frag)
    return not_served(r, DIHIP_PARAM_ERROR,
                      "gemm_lowp: the FRAG32 activation layout needs the small-batch kernel (see dihip_gemm_lowp_prefers_frag)");
  if (c.rowsq)
    return not_served(r, DIHIP_PARAM_ERROR, "gemm_lowp: this shape is not served by a kernel that takes deferred row norms");
  // context phase (M >= 64 rows): 128 x 256 workgroup tiles, A through LDS, every weight byte read once per 128 rows
  // (gemm_prefill_kernel.hpp).  DIHIP_GEMM_PREFILL=0 keeps the general kernel (A/B, diagnostics).
  static const bool prefill_on = !env_off("DIHIP_GEMM_PREFILL");
  if (prefill_on && c.pro == PRO_PLAIN && c.M >= 64 && (c.wbits == 4 || c.wbits == 8) && aligned && whole_groups &&
      (!dual || c.has_w1)) {
    r.prefill = prefill_tail_plan(c.wbits, c.M, c.N, c.K, c.group_size, dual);
    const PrefillTail& t = r.prefill;
    if (t.ksplit > 1 && !(c.ws_bytes >= t.slab_bytes && c.ws_aligned)) {  // the slab does not fit: the unsplit grid
      r.prefill.tail_cb = t.col_blocks;
      r.prefill.ksplit = 1;
      r.prefill.slab_bytes = 0;
    }
    const unsigned blocks = t.tail_cb * t.mblocks + (t.col_blocks - t.tail_cb) * t.mblocks * t.ksplit;
    r.mt = 0;
    set_launch(r, FAM_GEMM_PREFILL, blocks, 1, 1, PF_THREADS, c.wbits == 4 ? prefill_lds_bytes<4>() : prefill_lds_bytes<8>(),
               t.slab_bytes);
    return r;
  }
  r.gemm = make_plan(c.wbits, c.M, c.N, c.K, c.group_size, dual);
  const GemmPlan& p = r.gemm;
  if ((size_t)p.col_blocks * p.m_blocks * sizeof(unsigned) > GEMM_SYNC_BYTES)
    return not_served(r, DIHIP_EXCEED_LIMIT_ERROR, "gemm_lowp: too many tiles for the sync buffer");
  const size_t need = p.slab_bytes + (c.has_sync ? 0 : GEMM_SYNC_BYTES);  // no sync buffer: the counters follow the slab
  if (p.splitk > 1 && c.ws_bytes < need) return not_served(r, DIHIP_MEMORY_ERROR, "gemm_lowp: workspace too small", need);
  r.mt = p.MT;
  r.nt = p.NT;
  r.gpt = 0;  // the general kernel has no group-per-tile form
  set_launch(r, FAM_GEMM_LOWP, p.col_blocks, p.splitk, p.m_blocks, GEMM_THREADS, p.lds_bytes, p.slab_bytes);
  return r;
}

bool lowp_prefers_frag(int wbits, int M, int N, int K, int group_size, bool dual) {
  if (M <= 0 || N <= 0 || K <= 0) return false;
  return plan_gemm(GemmDesc::of_shape(wbits, DIHIP_BF16, PRO_PLAIN, dual ? EPI_SWIGLU : EPI_STD, M, N, K, group_size,
                                      DIHIP_ACT_ROWMAJOR, DIHIP_ACT_ROWMAJOR)).family == FAM_GEMV_BATCH;
}

bool lowp_frag_served(int wbits, int dtype, int M, int N, int K, int group_size, bool dual) {
  if (M <= 0 || N <= 0 || K <= 0) return false;
  return plan_gemm(GemmDesc::of_shape(wbits, dtype, PRO_PLAIN, dual ? EPI_SWIGLU : EPI_STD, M, N, K, group_size,
                                      DIHIP_ACT_FRAG32, DIHIP_ACT_FRAG32)).family != FAM_NONE;
}

}  // namespace dihip

using namespace dihip;

extern "C" {

size_t dihip_gemm_lowp_packed_weight_bytes(int wbits, int N, int K) {
  if ((wbits != 4 && wbits != 8) || N <= 0 || K <= 0) return 0;
  const LowpDims d = lowp_dims(wbits, N, K, -1);
  return (size_t)d.NTILES * d.KT * 64 * 16;
}

size_t dihip_gemm_lowp_packed_sz_bytes(int N, int K, int group_size) {
  if (N <= 0 || K <= 0) return 0;
  const LowpDims d = lowp_dims(4, N, K, group_size);  // Kp depends on wbits only through the tile: the larger padding
  return (size_t)d.Gp_packed * d.Np * 4;
}

size_t dihip_dense_packed_weight_bytes(int N, int K) {
  if (N <= 0 || K <= 0) return 0;
  const LowpDims d = lowp_dims(16, N, K, -1);
  return (size_t)d.NTILES * d.KT * 64 * 16;
}

size_t dihip_gemm_lowp_sync_bytes(void) { return GEMM_SYNC_BYTES; }

size_t dihip_gemm_lowp_workspace_bytes(int wbits, int M, int N, int K, int group_size) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  // sized for the dual (SwiGLU) form, the self-contained counter area and the M > 4 norm buffer
  const size_t slab = std::max(lowp_slab_bytes(wbits, M, N, K, group_size, false), lowp_slab_bytes(wbits, M, N, K, group_size, true));
  return slab + GEMM_SYNC_BYTES + (size_t)((M + 15) / 16 * 16) * K * 2 + 512;  // norm rows may be FRAG32
}

size_t dihip_dense_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return lowp_slab_bytes(16, M, N, K, -1, false) + GEMM_SYNC_BYTES + (size_t)M * K * 2 + 512;
}

// K parts per tail tile the context-phase GEMM of this shape is launched with on this GPU (1: no tail split; diagnostics / tests)
int dihip_gemm_prefill_tail_parts(int wbits, int M, int N, int K, int group_size, int dual) {
  if (M < 64 || N <= 0 || K <= 0) return 1;
  return prefill_tail_plan(wbits, M, N, K, group_size, dual != 0).ksplit;
}

int dihip_gemm_lowp_prefers_frag(int wbits, int M, int N, int K, int group_size, int dual) {
  return lowp_prefers_frag(wbits, M, N, K, group_size, dual != 0) ? 1 : 0;
}

// can a prenorm GEMM (dual = 0) / SwiGLU pair (dual = 1) of this shape take deferred row norms?
int dihip_prenorm_rowsq_supported(int wbits, int M, int N, int K, int group_size, int dual, int dtype, int x_layout) {
  static const bool on = !env_off("DIHIP_DEFER_RMSNORM");  // =0: never (A/B; callers then keep the norm launch)
  if (!on || M <= 0 || N <= 0 || K <= 0) return 0;
  GemmDesc c = GemmDesc::of_shape(wbits, dtype, PRO_PLAIN, dual ? EPI_SWIGLU : EPI_STD, M, N, K, group_size, x_layout, DIHIP_ACT_ROWMAJOR);
  c.rowsq = true;
  return plan_gemm(c).family != FAM_NONE ? 1 : 0;
}

int dihip_debug_gemv_plan(int wbits, int M, int N, int K, int group_size, int dual, int* blocks, int* upb, int* wk, int* wn,
                          size_t* lds_bytes) {
  const GemvPlan p = make_gemv_plan(wbits, M, N, K, group_size, dual != 0);
  if (!p.ok) return DIHIP_PARAM_ERROR;
  if (blocks) *blocks = p.blocks;
  if (upb) *upb = p.upb;
  if (wk) *wk = p.WK;
  if (wn) *wn = p.WN;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return DIHIP_SUCCESS;
}

int dihip_debug_gemm_route(int wbits, int dtype, int pro, int epi, int M, int N, int K, int group_size, int x_layout,
                           int y_layout, int flags, long long* out) {
  DIHIP_REQUIRE(out && M > 0 && N > 0 && K > 0 && (wbits == 4 || wbits == 8 || wbits == 16), DIHIP_PARAM_ERROR,
                "debug_gemm_route: bad argument");
  GemmDesc c = GemmDesc::of_shape(wbits, dtype, pro, epi, M, N, K, group_size, x_layout, y_layout);
  c.rowsq = flags & DIHIP_ROUTE_ROWSQ;
  c.n_gamma = flags & (DIHIP_ROUTE_NORM | DIHIP_ROUTE_PRENORM);
  c.n_rowsq_bytes = (flags & DIHIP_ROUTE_PRENORM) ? dihip_rowsq_bytes() : 0;
  if (flags & DIHIP_ROUTE_NO_WS) c.ws_bytes = 0;
  if (flags & DIHIP_ROUTE_NO_SYNC) c.has_sync = false;
  if (flags & DIHIP_ROUTE_UNALIGNED) c.x_aligned = c.gamma_aligned = c.ws_aligned = false;
  const GemmRoute r = plan_gemm(c);
  const long long v[DIHIP_ROUTE_FIELDS] = {r.family, r.mt, r.nt, r.pro, r.epi, r.gpt, r.rs, r.grid[0], r.grid[1], r.grid[2],
                                           r.threads, (long long)r.lds_bytes, (long long)r.slab_bytes, r.ncu,
                                           r.norm_in_reduce ? 1 : r.prenorm_parts > 0 ? 2 : 0, r.status};
  std::copy(v, v + DIHIP_ROUTE_FIELDS, out);
  return DIHIP_SUCCESS;
}

}  // extern "C"
