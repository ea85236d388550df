// gemm_lowp.hip -- weight re-layout kernels, kernel launch and the C-ABI entry points of the weight-only GEMM
// (include/dashinfer_hip.h section 1).  Which kernel serves a call, and with which grid: gemm_lowp_plan.hpp.
#include <algorithm>

#include "gemm_lowp_plan.hpp"
#include "gemm_lowp_launch.hpp"
#include "gemv_stream_kernel.hpp"
#include "gemm_prefill_kernel.hpp"
#include "gemv_batch_kernel.hpp"
#include "gemm_kslice_kernel.hpp"
#include "gemm_panel_kernel.hpp"

namespace dihip {

// ------------------------------------------------------------------------------------------
// "dihip tile-major" weight layout
//   W4: Kp = roundup(K,128), Np = roundup(N,16); 16-byte chunk index ((nt*KT + kt)*64 + lane),
//       lane = kb*16 + n%16, kb = (k%32)/8; dword ks = (k%128)/32 of the chunk holds the 8
//       nibbles j = k%8 at bit 4*(j/2) + 16*(j%2).
//   W8: Kp = roundup(K,64); chunk byte ks*8 + j = u8(q + 128), ks = (k%64)/32.
//   padding (k >= K or n >= N) is zero.
// (scale, zero): uint32 [NTILES][Gp][16] (column-tile major: the parameters a wave needs next to
//   a weight chunk are 64 contiguous bytes, consecutive groups of a tile are adjacent), lo16 =
//   scale bits, hi16 = zero bits (FT), zero padded; Gp = max(G, ceil(Kp / group)).
// ------------------------------------------------------------------------------------------
__global__ void pack_w4_kernel(const uint8_t* __restrict__ wq, uint32_t* __restrict__ out, int N,
                               int K, int KT, int NTILES) {
  const size_t total = (size_t)NTILES * KT * 64 * 4;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int ks = idx & 3;
    const int lane = (idx >> 2) & 63;
    const size_t tk = idx >> 8;
    const int kt = (int)(tk % KT), nt = (int)(tk / KT);
    const int n = nt * 16 + (lane & 15), kb = lane >> 4;
    const int NP = (N + 1) / 2;
    uint32_t d = 0;
    if (n < N) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = kt * 128 + ks * 32 + kb * 8 + j;
        if (k < K) {
          const uint8_t b = wq[(size_t)k * NP + (n >> 1)];
          const uint32_t q = (n & 1) ? (b >> 4) : (b & 0xF);  // convert_4bit.h:9-16
          d |= q << (4 * (j >> 1) + 16 * (j & 1));
        }
      }
    }
    out[idx] = d;
  }
}

__global__ void pack_w8_kernel(const int8_t* __restrict__ wq, uint32_t* __restrict__ out, int N,
                               int K, int KT, int NTILES) {
  const size_t total = (size_t)NTILES * KT * 64 * 4;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int dw = idx & 3;
    const int lane = (idx >> 2) & 63;
    const size_t tk = idx >> 8;
    const int kt = (int)(tk % KT), nt = (int)(tk / KT);
    const int n = nt * 16 + (lane & 15), kb = lane >> 4;
    const int ks = dw >> 1, j0 = (dw & 1) * 4;
    uint32_t d = 0;
    if (n < N) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = kt * 64 + ks * 32 + kb * 8 + j0 + j;
        if (k < K) d |= (uint32_t)(uint8_t)((int)wq[(size_t)k * N + n] + 128) << (8 * j);
      }
    }
    out[idx] = d;
  }
}

// W16: chunk = the 8 consecutive k (FT elements) of column n for k-step kt, lane = kb*16 + n%16
__global__ void pack_w16_kernel(const uint16_t* __restrict__ w, uint32_t* __restrict__ out, int N, int K, int KT,
                                int NTILES) {
  const size_t total = (size_t)NTILES * KT * 64 * 4;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int dw = idx & 3;
    const int lane = (idx >> 2) & 63;
    const size_t tk = idx >> 8;
    const int kt = (int)(tk % KT), nt = (int)(tk / KT);
    const int n = nt * 16 + (lane & 15), kb = lane >> 4;
    const int k = kt * 32 + kb * 8 + dw * 2;
    uint32_t d = 0;
    if (n < N) {
      if (k < K) d |= (uint32_t)w[(size_t)k * N + n];
      if (k + 1 < K) d |= (uint32_t)w[(size_t)(k + 1) * N + n] << 16;
    }
    out[idx] = d;
  }
}

__global__ void pack_sz_kernel(const uint16_t* __restrict__ s, const uint16_t* __restrict__ z,
                               uint32_t* __restrict__ out, int N, int Np, int G, int Gp) {
  const size_t total = (size_t)Gp * Np;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int col = (int)(idx & 15);
    const int g = (int)((idx >> 4) % Gp);
    const int n = (int)((idx >> 4) / Gp) * 16 + col;
    uint32_t v = 0;
    if (n < N && g < G) v = (uint32_t)s[(size_t)g * N + n] | ((uint32_t)z[(size_t)g * N + n] << 16);
    out[idx] = v;
  }
}

// f32 hidden rows -> FT normalised rows (used by the fused entry points when M > 4); frag_mt > 0: FRAG32 output.
// One workgroup per row, the row stays in registers (one 16-byte load per 4 columns, all in flight together):
// a single round trip instead of two dependent passes over h.  cols % 4 == 0, cols <= 256 * 4 * VPT.
template <int FT, int VPT, int THREADS>
__global__ __launch_bounds__(THREADS) void rmsnorm_f32_to_ft_kernel(uint16_t* __restrict__ y, const float* __restrict__ h,
                                                                const void* __restrict__ gamma, float eps, int cols,
                                                                int frag_mt) {
  __shared__ float red[THREADS / 64];
  const int row = blockIdx.x, tid = threadIdx.x;
  const f32x4_t* hr = reinterpret_cast<const f32x4_t*>(h + (size_t)row * cols);
  const int nvec = cols >> 2;
  f32x4_t v[VPT];
  u32x2_t gm[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int c = tid + i * THREADS;
    v[i] = c < nvec ? hr[c] : f32x4_t{0.f, 0.f, 0.f, 0.f};
    gm[i] = c < nvec ? reinterpret_cast<const u32x2_t*>(gamma)[c] : u32x2_t{0u, 0u};
  }
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) ss += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
  ss = wave_sum(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  float tot = red[0];
#pragma unroll
  for (int w = 1; w < THREADS / 64; ++w) tot += red[w];
  const float rstd = 1.f / sqrtf(tot / (float)cols + eps);
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int c = tid + i * THREADS;
    if (c < nvec) {
      const float g0 = ft_bits_to_f32<FT>(gm[i][0] & 0xFFFFu), g1 = ft_bits_to_f32<FT>(gm[i][0] >> 16);
      const float g2 = ft_bits_to_f32<FT>(gm[i][1] & 0xFFFFu), g3 = ft_bits_to_f32<FT>(gm[i][1] >> 16);
      const uint32_t lo = f32_to_ft_bits<FT>((g0 * v[i][0]) * rstd) | (f32_to_ft_bits<FT>((g1 * v[i][1]) * rstd) << 16);
      const uint32_t hi = f32_to_ft_bits<FT>((g2 * v[i][2]) * rstd) | (f32_to_ft_bits<FT>((g3 * v[i][3]) * rstd) << 16);
      const int k = c * 4;  // 4 consecutive columns stay adjacent in both layouts
      const size_t idx = frag_mt ? act_frag_index(row, k, frag_mt) : (size_t)row * cols + k;
      *reinterpret_cast<u32x2_t*>(y + idx) = u32x2_t{lo, hi};
    }
  }
}

// any width (two passes over the row)
template <int FT>
__global__ __launch_bounds__(256) void rmsnorm_f32_to_ft_wide_kernel(uint16_t* __restrict__ y, const float* __restrict__ h,
                                                                     const void* __restrict__ gamma, float eps, int cols,
                                                                     int frag_mt) {
  __shared__ float red[4];
  const float* hr = h + (size_t)blockIdx.x * cols;
  float ss = 0.f;
  for (int k = threadIdx.x; k < cols; k += 256) ss += hr[k] * hr[k];
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float rstd = 1.f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)cols + eps);
  for (int k = threadIdx.x; k < cols; k += 256) {
    const size_t idx = frag_mt ? act_frag_index((int)blockIdx.x, k, frag_mt) : (size_t)blockIdx.x * cols + k;
    y[idx] = (uint16_t)f32_to_ft_bits<FT>((load_ft<FT>(gamma, k) * hr[k]) * rstd);
  }
}

// row-major [M, K] 16-bit <-> FRAG32 (tests / callers that produce activations outside this library)
__global__ void act_frag_convert_kernel(uint16_t* __restrict__ dst, const uint16_t* __restrict__ src, int M, int K, int mt,
                                        int to_frag) {
  const size_t total = (size_t)M * K;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(i / K), k = (int)(i - (size_t)m * K);
    const size_t f = act_frag_index(m, k, mt);
    if (to_frag) dst[f] = src[i];
    else dst[i] = src[f];
  }
}

// ------------------------------------------------------------------------------------------
// launch: kernel arguments and the thunk tables (instantiations: *_inst_*.hip)
// ------------------------------------------------------------------------------------------
// operands and shape: what every launch has, the expert slots (run_gemv_slots) included
template <class Args>
static void fill_operands(Args& g, const void* x, const void* w0, const void* sz0, const void* w1, const void* sz1, void* y, int M,
                          int N, const LowpDims& d) {
  g.w0 = reinterpret_cast<const u32x4_t*>(w0);
  g.w1 = reinterpret_cast<const u32x4_t*>(w1);
  g.sz0 = reinterpret_cast<const uint32_t*>(sz0);
  g.sz1 = reinterpret_cast<const uint32_t*>(sz1);
  g.x = x;
  g.y = y;
  g.ldy = N;
  g.alpha = 1.f;
  g.act = DIHIP_ACT_NONE;
  g.M = M;
  g.N = N;
  g.KT = d.KT;
  g.NTILES = d.NTILES;
  g.Gp = d.Gp_packed;
}
// the fields every family's argument struct has
template <class Args>
static void fill_common(Args& g, const GemmCall& c, const LowpDims& d) {
  fill_operands(g, c.x, c.w0, c.sz0, c.w1, c.sz1, c.y, c.M, c.N, d);
  g.bias = c.bias;
  g.residual = c.residual;
  g.h_res = c.h_res;
  g.h_out = c.h_out;
  g.alpha = c.alpha;
  g.act = c.act;
}
// deferred row norms handed in (GembArgs / PanelArgs)
template <class Args>
static void fill_rowsq(Args& g, const GemmCall& c) {
  g.rowsq = c.rowsq;
  g.rowsq_parts = c.rowsq_parts;
  g.rowsq_eps = c.rowsq_eps;
}
// the K-slice and the panel kernel share their arguments
static void fill_panel(PanelArgs& g, const GemmCall& c, const LowpDims& d, const GemmRoute& r, int nslices) {
  fill_common(g, c, d);
  g.K = c.K;
  g.ktpg = d.ktpg;
  g.nslices = nslices;
  g.slab = reinterpret_cast<float*>(c.ws);
  g.yfrag = c.y_layout == DIHIP_ACT_FRAG32;
  if (r.norm_in_reduce) {
    g.n_gamma = c.n_gamma;
    g.n_eps = c.n_eps;
    g.n_out = c.n_out;
    g.n_frag_mt = c.n_frag_mt;
  }
  if (c.rowsq) fill_rowsq(g, c);  // applied in the epilogue (unsplit K) or in the slab reduction
}

#define DIHIP_BOTH_FT(CASES) CASES(DIHIP_BF16) CASES(DIHIP_F16)

static hipError_t launch_route_gemv(const GemmCall& c, const GemmRoute& r, const GemvArgs& g, hipStream_t s) {
#define GO(W_, FT_, MR_, PRO_, EPI_, G_)                                                                     \
  if (c.wbits == W_ && c.dtype == FT_ && r.mt == MR_ && r.pro == PRO_ && r.epi == EPI_ && r.gpt == G_) \
    return launch_gemv_stream<W_, FT_, MR_, PRO_, EPI_, G_>(g, r.grid[0], r.lds_bytes, s);
#define FORMS(W_, FT_, G_) \
  GO(W_, FT_, 1, PRO_PLAIN, EPI_STD, G_) \
  GO(W_, FT_, 4, PRO_PLAIN, EPI_STD, G_) \
  GO(W_, FT_, 1, PRO_RMSNORM, EPI_STD, G_) \
  GO(W_, FT_, 4, PRO_RMSNORM, EPI_STD, G_) \
  GO(W_, FT_, 1, PRO_RMSNORM, EPI_SWIGLU, G_) \
  GO(W_, FT_, 4, PRO_RMSNORM, EPI_SWIGLU, G_) \
  GO(W_, FT_, 1, PRO_PLAIN, EPI_SWIGLU, G_) \
  GO(W_, FT_, 4, PRO_PLAIN, EPI_SWIGLU, G_) \
  GO(W_, FT_, 1, PRO_PLAIN, EPI_ADDTO, G_) \
  GO(W_, FT_, 4, PRO_PLAIN, EPI_ADDTO, G_) \
  GO(W_, FT_, 1, PRO_RMSNORM, EPI_ADDTO, G_) \
  GO(W_, FT_, 4, PRO_RMSNORM, EPI_ADDTO, G_)
#define CASES(FT_) FORMS(4, FT_, 0) FORMS(4, FT_, 1) FORMS(8, FT_, 0) FORMS(8, FT_, 1) FORMS(16, FT_, 0)
  DIHIP_BOTH_FT(CASES)
#undef CASES
#undef FORMS
#undef GO
  return hipErrorInvalidValue;
}

static hipError_t launch_route_kslice(const GemmCall& c, const GemmRoute& r, const PanelArgs& g, hipStream_t s) {
  const int groups = r.kslice.groups, waves = r.kslice.waves;
#define GO(W_, FT_, MT_, EPI_, G_)                                                                   \
  if (c.wbits == W_ && c.dtype == FT_ && r.mt == MT_ && r.epi == EPI_ && r.gpt == G_ && !r.rs) \
    return launch_gemm_kslice<W_, FT_, MT_, EPI_, G_>(g, groups, waves, s);
#define GO_RS(W_, MT_, EPI_, G_) /* the deferred-RMSNorm consumer has its own instantiations (bf16) */ \
  if (c.wbits == W_ && r.mt == MT_ && r.epi == EPI_ && r.gpt == G_ && r.rs) return launch_gemm_kslice_rs<W_, MT_, EPI_, G_>(g, groups, waves, s);
#define FORMS(W_, FT_, G_)                                                                                      \
  GO(W_, FT_, 1, EPI_STD, G_) GO(W_, FT_, 2, EPI_STD, G_) GO(W_, FT_, 1, EPI_SWIGLU, G_) GO(W_, FT_, 2, EPI_SWIGLU, G_) \
  GO(W_, FT_, 1, EPI_ADDTO, G_) GO(W_, FT_, 2, EPI_ADDTO, G_)
#define FORMS_RS(W_, G_) GO_RS(W_, 1, EPI_STD, G_) GO_RS(W_, 2, EPI_STD, G_) GO_RS(W_, 1, EPI_SWIGLU, G_) GO_RS(W_, 2, EPI_SWIGLU, G_)
#define CASES(FT_) FORMS(4, FT_, 0) FORMS(4, FT_, 1) FORMS(8, FT_, 0)  // W8 with a group per k-tile (g64) is excluded by the plan
  DIHIP_BOTH_FT(CASES)
  FORMS_RS(4, 0) FORMS_RS(4, 1) FORMS_RS(8, 0)
#undef CASES
#undef FORMS_RS
#undef FORMS
#undef GO_RS
#undef GO
  return hipErrorInvalidValue;
}

static hipError_t launch_route_panel(const GemmCall& c, const GemmRoute& r, const PanelArgs& g, hipStream_t s) {
#define GO(W_, FT_, MT_, EPI_, G_)                                                         \
  if (c.wbits == W_ && c.dtype == FT_ && r.mt == MT_ && r.epi == EPI_ && r.gpt == G_) \
    return launch_gemm_panel<W_, FT_, MT_, EPI_, G_>(g, r.panel.panels, s);
#define FORMS(W_, FT_, G_)                                                                                      \
  GO(W_, FT_, 1, EPI_STD, G_) GO(W_, FT_, 2, EPI_STD, G_) GO(W_, FT_, 1, EPI_SWIGLU, G_) GO(W_, FT_, 2, EPI_SWIGLU, G_) \
  GO(W_, FT_, 1, EPI_ADDTO, G_) GO(W_, FT_, 2, EPI_ADDTO, G_)
#define CASES(FT_) FORMS(4, FT_, 0) FORMS(4, FT_, 1) FORMS(8, FT_, 0) FORMS(8, FT_, 1)
  DIHIP_BOTH_FT(CASES)
#undef CASES
#undef FORMS
#undef GO
  return hipErrorInvalidValue;
}

static hipError_t launch_route_gemb(const GemmCall& c, const GemmRoute& r, const GembArgs& g, hipStream_t s) {
#define GO(W_, FT_, MT_, NT_, EPI_, G_)                                                                    \
  if (c.wbits == W_ && c.dtype == FT_ && r.mt == MT_ && r.nt == NT_ && r.epi == EPI_ && r.gpt == G_) \
    return launch_gemv_batch<W_, FT_, MT_, NT_, EPI_, G_>(g, r.gemb.blocks, s);
#define EPIS(W_, FT_, MT_, NT_, G_) GO(W_, FT_, MT_, NT_, EPI_STD, G_) GO(W_, FT_, MT_, NT_, EPI_SWIGLU, G_) GO(W_, FT_, MT_, NT_, EPI_ADDTO, G_)
#define FORMS(W_, FT_, G_) EPIS(W_, FT_, 1, 1, G_) EPIS(W_, FT_, 2, 1, G_) EPIS(W_, FT_, 1, 2, G_) EPIS(W_, FT_, 2, 2, G_)
#define CASES(FT_) FORMS(4, FT_, 0) FORMS(4, FT_, 1) FORMS(8, FT_, 0) FORMS(8, FT_, 1)
  DIHIP_BOTH_FT(CASES)
#undef CASES
#undef FORMS
#undef EPIS
#undef GO
  return hipErrorInvalidValue;
}

static hipError_t launch_route_prefill(const GemmCall& c, const GemmRoute& r, const PrefillArgs& g, hipStream_t s) {
#define GO(W_, FT_, EPI_, G_) \
  if (c.wbits == W_ && c.dtype == FT_ && r.epi == EPI_ && r.gpt == G_) return launch_gemm_prefill<W_, FT_, EPI_, G_>(g, r.grid[0], s);
#define FORMS(W_, FT_) GO(W_, FT_, EPI_STD, 0) GO(W_, FT_, EPI_STD, 1) GO(W_, FT_, EPI_SWIGLU, 0) GO(W_, FT_, EPI_SWIGLU, 1) \
  GO(W_, FT_, EPI_ADDTO, 0) GO(W_, FT_, EPI_ADDTO, 1)
#define CASES(FT_) FORMS(4, FT_) FORMS(8, FT_)
  DIHIP_BOTH_FT(CASES)
#undef CASES
#undef FORMS
#undef GO
  return hipErrorInvalidValue;
}

static hipError_t launch_route_gemm(const GemmCall& c, const GemmRoute& r, const GemmArgs& a, hipStream_t s) {
  const dim3 grid(r.grid[0], r.grid[1], r.grid[2]);
#define GO(W_, FT_, MT_, NT_, PRO_, EPI_)                                                                   \
  if (c.wbits == W_ && c.dtype == FT_ && r.mt == MT_ && r.nt == NT_ && r.pro == PRO_ && r.epi == EPI_) \
    return launch_gemm_lowp<W_, FT_, MT_, NT_, PRO_, EPI_>(a, grid, r.lds_bytes, s);
#define FORMS(W_, FT_) \
  GO(W_, FT_, 1, 2, PRO_PLAIN, EPI_STD) \
  GO(W_, FT_, 1, 4, PRO_PLAIN, EPI_STD) \
  GO(W_, FT_, 2, 2, PRO_PLAIN, EPI_STD) \
  GO(W_, FT_, 2, 4, PRO_PLAIN, EPI_STD) /* fused decode-step forms: */ \
  GO(W_, FT_, 1, 2, PRO_RMSNORM, EPI_STD) \
  GO(W_, FT_, 1, 4, PRO_RMSNORM, EPI_STD) \
  GO(W_, FT_, 1, 4, PRO_RMSNORM, EPI_SWIGLU) \
  GO(W_, FT_, 1, 4, PRO_PLAIN, EPI_SWIGLU) \
  GO(W_, FT_, 2, 4, PRO_PLAIN, EPI_SWIGLU) \
  GO(W_, FT_, 1, 2, PRO_PLAIN, EPI_ADDTO) \
  GO(W_, FT_, 1, 4, PRO_PLAIN, EPI_ADDTO) \
  GO(W_, FT_, 2, 2, PRO_PLAIN, EPI_ADDTO) \
  GO(W_, FT_, 2, 4, PRO_PLAIN, EPI_ADDTO)
#define FORMS_DENSE(FT_) /* unquantised weights: lm_head (rmsnorm prologue for M <= 4, f32 logits out) and dense Gemm */ \
  GO(16, FT_, 1, 4, PRO_RMSNORM, EPI_ADDTO) \
  GO(16, FT_, 1, 4, PRO_PLAIN, EPI_ADDTO) \
  GO(16, FT_, 2, 4, PRO_PLAIN, EPI_ADDTO) \
  GO(16, FT_, 1, 4, PRO_PLAIN, EPI_STD) \
  GO(16, FT_, 2, 4, PRO_PLAIN, EPI_STD)
#define CASES(FT_) FORMS(4, FT_) FORMS(8, FT_) FORMS_DENSE(FT_)
  DIHIP_BOTH_FT(CASES)
#undef CASES
#undef FORMS_DENSE
#undef FORMS
#undef GO
  return hipErrorInvalidValue;
}
#undef DIHIP_BOTH_FT

static const char* const FAMILY_NAME[] = {"none", "gemv_stream", "gemm_kslice", "gemm_panel", "gemv_batch", "gemm_prefill", "gemm_lowp"};

// validate, plan, fill the family's arguments, launch
static int run_gemm(hipStream_t stream, const GemmCall& c) {
  DIHIP_REQUIRE(c.M >= 0 && c.N > 0 && c.K > 0, DIHIP_PARAM_ERROR, "gemm_lowp: bad shape M=%d N=%d K=%d",
                c.M, c.N, c.K);
  if (c.M == 0) return DIHIP_SUCCESS;  // empty batch
  DIHIP_REQUIRE(c.dtype == DIHIP_BF16 || c.dtype == DIHIP_F16, DIHIP_PARAM_ERROR,
                "gemm_lowp: activation type must be FLOAT16 or BFLOAT16 (gemm_a16w8.cpp:21-125)");
  DIHIP_REQUIRE(c.group_size <= 0 || c.group_size % 32 == 0, DIHIP_PARAM_ERROR,
                "gemm_lowp: GroupSize %d must be a multiple of 32", c.group_size);
  DIHIP_REQUIRE(c.x && c.w0 && (c.sz0 || c.wbits == 16), DIHIP_PARAM_ERROR, "gemm_lowp: null input pointer");
  if (c.n_parts) *c.n_parts = 0;

  const GemmRoute r = plan_gemm(describe(c));
  if (r.family == FAM_NONE) {
    if (r.status == DIHIP_MEMORY_ERROR) set_last_error("%s (%zu < %zu)", r.error, c.ws ? c.ws_bytes : (size_t)0, r.need_bytes);
    else set_last_error("%s", r.error);
    return r.status;
  }
  if (c.n_done && (r.norm_in_reduce || r.prenorm_parts > 0)) *c.n_done = true;
  if (r.prenorm_parts > 0) *c.n_parts = r.prenorm_parts;

  const LowpDims d = lowp_dims(c.wbits, c.N, c.K, c.group_size);
  hipError_t e = hipErrorInvalidValue;
  switch (r.family) {
    case FAM_GEMV_STREAM: {
      GemvArgs g{};
      fill_common(g, c, d);
      g.ldx = c.ldx;
      g.gamma = c.gamma;
      g.eps = c.eps;
      g.K = c.K;
      fill_gemv_plan(&g, r.gemv, d, r.gemv.blocks);
      g.trace = debug_trace_buffer((size_t)r.gemv.blocks * GEMV_WAVES * 64);
      e = launch_route_gemv(c, r, g, stream);
      break;
    }
    case FAM_GEMM_KSLICE: {
      PanelArgs g{};
      fill_panel(g, c, d, r, r.kslice.nslices);
      g.nunits = r.kslice.nunits;
      g.trace = debug_trace_buffer((size_t)r.kslice.groups * r.kslice.nslices * KSL_WAVES * 64);
      e = launch_route_kslice(c, r, g, stream);
      break;
    }
    case FAM_GEMM_PANEL: {
      PanelArgs g{};
      fill_panel(g, c, d, r, r.panel.nslices);
      g.ktps = r.panel.ktps;
      e = launch_route_panel(c, r, g, stream);
      break;
    }
    case FAM_GEMV_BATCH: {
      DIHIP_REQUIRE(!c.rowsq || c.rowsq_parts <= 16 * (GEMB_THREADS / 32), DIHIP_PARAM_ERROR, "gemv_batch: more than %d row-norm parts",
                    16 * (GEMB_THREADS / 32));
      GembArgs g{};
      fill_common(g, c, d);
      g.ldx = c.ldx;
      g.K = c.K;
      g.ktpg = d.ktpg;
      g.kgroups = d.group ? (d.KT + g.ktpg - 1) / g.ktpg : d.KT;
      g.xfrag = c.x_layout == DIHIP_ACT_FRAG32;
      g.yfrag = c.y_layout == DIHIP_ACT_FRAG32;
      g.upb = r.gemb.upb;
      if (r.prenorm_parts > 0) {  // deferred RMSNorm, producer side
        g.n_gamma = c.n_gamma;
        g.n_out = c.n_out;
        g.n_frag_mt = c.n_frag_mt;
        g.n_rowsq = c.n_rowsq;
      }
      if (c.rowsq) fill_rowsq(g, c);
      e = launch_route_gemb(c, r, g, stream);
      break;
    }
    case FAM_GEMM_PREFILL: {
      PrefillArgs g{};
      fill_common(g, c, d);
      g.ldx = c.ldx;
      g.ktpg = d.ktpg;
      g.col_blocks = r.prefill.col_blocks;
      g.tail_cb = r.prefill.tail_cb;
      g.ksplit = r.prefill.ksplit;
      if (r.prefill.ksplit > 1) g.slab = reinterpret_cast<float*>(c.ws);
      g.trace = debug_trace_buffer((size_t)r.grid[0] * PF_WAVES * 4 * 8 * sizeof(unsigned long long));
      e = launch_route_prefill(c, r, g, stream);
      break;
    }
    default: {
      GemmArgs a{};
      fill_common(a, c, d);
      a.ldx = c.ldx;
      a.gamma = c.gamma;
      a.eps = c.eps;
      a.K = c.K;
      a.Np = d.Np;
      a.ksteps_per_group = d.group ? d.group / 32 : (1 << 30);
      a.splitk = r.gemm.splitk;
      a.ktiles_per_split = r.gemm.ktiles_per_split;
      a.kslice_tiles = r.gemm.kslice_tiles;
      a.slabs = reinterpret_cast<float*>(c.ws);
      a.counters = reinterpret_cast<unsigned*>(c.sync);
      if (r.gemm.splitk > 1 && !c.sync) {  // self-contained: the counters follow the slab and are cleared per call
        a.counters = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(c.ws) + r.slab_bytes);
        DIHIP_CHECK_HIP(hipMemsetAsync(a.counters, 0, (size_t)r.grid[0] * r.grid[2] * sizeof(unsigned), stream), DIHIP_RUNTIME_ERROR);
      }
      e = launch_route_gemm(c, r, a, stream);
    }
  }
  DIHIP_REQUIRE(e == hipSuccess, e == hipErrorInvalidValue ? DIHIP_PARAM_ERROR : DIHIP_RUNTIME_ERROR,
                "%s: launch failed (wbits=%d dtype=%d M=%d mt=%d nt=%d pro=%d epi=%d gpt=%d): %s", FAMILY_NAME[r.family], c.wbits,
                c.dtype, c.M, r.mt, r.nt, r.pro, r.epi, r.gpt, hipGetErrorString(e));
  return DIHIP_SUCCESS;
}

int run_gemv_slots(hipStream_t stream, int wbits, int epi, const void* x, int ldx, int x_div, const void* w0, const void* sz0,
                   const void* w1, const void* sz1, void* y, int N, int K, int group_size, const int* slot_expert, int nslots,
                   const int* group_rows, const int* group_nrows) {
  const bool grouped = group_rows != nullptr;  // slot_expert / nslots then enumerate groups of <= 4 slots (moe.hip)
  const bool dual = epi == EPI_SWIGLU;
  const LowpDims d = lowp_dims(wbits, N, K, group_size);
  DIHIP_REQUIRE(K == d.Kp && (d.group == 0 || d.group % d.KTILE == 0), DIHIP_PARAM_ERROR,
                "moe: K = %d must be a multiple of the k-tile (%d) and groups whole k-tiles", K, d.KTILE);
  // slots multiply the grid: about one workgroup per CU over the whole launch, at most 8 units per workgroup
  int ncu = cached_num_cus();
  if (ncu <= 0) ncu = 256;
  const int want = std::max((d.NTILES + 7) / 8, (ncu + nslots - 1) / nslots);
  const GemvPlan gp = make_gemv_plan(wbits, grouped ? 4 : 1, N, K, group_size, dual, want);
  DIHIP_REQUIRE(gp.ok && gp.lds_bytes <= 64 * 1024, DIHIP_PARAM_ERROR, "moe: unsupported expert shape N=%d K=%d", N, K);
  GemvArgs g{};
  fill_operands(g, x, w0, sz0, w1, sz1, y, grouped ? 4 : 1, N, d);
  g.ldx = ldx;
  g.K = K;
  fill_gemv_plan(&g, gp, d, gp.blocks);
  g.slot_rows = group_rows;
  g.slot_nrows = group_nrows;
  g.slot_expert = slot_expert;
  g.w_estride = (size_t)d.NTILES * d.KT * 64;       // u32x4 per expert
  g.sz_estride = (size_t)d.NTILES * g.Gp * 16;      // u32 per expert
  g.x_div = x_div;
  g.nslots = nslots;
  const bool gpt = gp.ktpg == 1;
  hipError_t e = hipErrorInvalidValue;
#define SLOT_GO(W_, EPI_, G_)                                                                                          \
  if (wbits == W_ && epi == EPI_ && (int)gpt == G_)                                                                    \
    e = grouped ? launch_gemv_slots<W_, DIHIP_BF16, EPI_, G_, 4>(g, gp.blocks, gp.lds_bytes, stream)                   \
                : launch_gemv_slots<W_, DIHIP_BF16, EPI_, G_, 1>(g, gp.blocks, gp.lds_bytes, stream);
  SLOT_GO(8, EPI_SWIGLU, 0) SLOT_GO(8, EPI_STD, 0) SLOT_GO(8, EPI_SWIGLU, 1) SLOT_GO(8, EPI_STD, 1)
  SLOT_GO(4, EPI_SWIGLU, 0) SLOT_GO(4, EPI_STD, 0) SLOT_GO(4, EPI_SWIGLU, 1) SLOT_GO(4, EPI_STD, 1)
#undef SLOT_GO
  DIHIP_REQUIRE(e == hipSuccess, DIHIP_RUNTIME_ERROR, "moe: expert GEMV launch failed: %s", hipGetErrorString(e));
  return DIHIP_SUCCESS;
}

int prefill_grouped_col_blocks(int N, bool dual) {
  const int tpb = dual ? PF_WN * PF_CW / 2 : PF_WN * PF_CW;
  return ((N + 15) / 16 + tpb - 1) / tpb;
}

int run_prefill_grouped(hipStream_t stream, int wbits, int epi, const void* x, int ldx, int x_div, const void* w0, const void* sz0,
                        const void* w1, const void* sz1, void* y, int N, int K, int group_size, const int* tiles, const int* ntiles,
                        const int* sorted_slot, int max_tiles) {
  const LowpDims d = lowp_dims(wbits, N, K, group_size);
  DIHIP_REQUIRE(K == d.Kp && (d.group == 0 || d.group % d.KTILE == 0) && ldx % 8 == 0, DIHIP_PARAM_ERROR,
                "moe: K = %d must be a multiple of the k-tile (%d) and groups whole k-tiles", K, d.KTILE);
  PrefillArgs g{};
  fill_operands(g, x, w0, sz0, w1, sz1, y, 0, N, d);
  g.ldx = ldx;
  g.ktpg = d.ktpg;
  g.col_blocks = prefill_grouped_col_blocks(N, epi == EPI_SWIGLU);
  g.tail_cb = g.col_blocks;  // no tail split
  g.ksplit = 1;
  g.g_tiles = tiles;
  g.g_ntiles = ntiles;
  g.g_sorted = sorted_slot;
  g.g_max_tiles = max_tiles;
  g.g_x_div = x_div;
  g.g_w_estride = (size_t)d.NTILES * d.KT * 64;
  g.g_sz_estride = (size_t)d.NTILES * g.Gp * 16;
  DIHIP_REQUIRE((size_t)max_tiles * g.col_blocks <= 0x7FFFFFFFu, DIHIP_EXCEED_LIMIT_ERROR, "moe: %d row tiles x %d column blocks exceed one launch",
                max_tiles, g.col_blocks);
  const bool gpt = d.group == d.KTILE;  // every k-tile is one quantisation group
  hipError_t e = hipErrorInvalidValue;
#define GROUPED_GO(W_, EPI_, G_) \
  if (wbits == W_ && epi == EPI_ && (int)gpt == G_) e = launch_gemm_prefill_grouped<W_, DIHIP_BF16, EPI_, G_>(g, stream);
  GROUPED_GO(8, EPI_SWIGLU, 0) GROUPED_GO(8, EPI_STD, 0) GROUPED_GO(8, EPI_SWIGLU, 1) GROUPED_GO(8, EPI_STD, 1)
  GROUPED_GO(4, EPI_SWIGLU, 0) GROUPED_GO(4, EPI_STD, 0) GROUPED_GO(4, EPI_SWIGLU, 1) GROUPED_GO(4, EPI_STD, 1)
#undef GROUPED_GO
  DIHIP_REQUIRE(e == hipSuccess, DIHIP_RUNTIME_ERROR, "moe: grouped expert GEMM launch failed: %s", hipGetErrorString(e));
  return DIHIP_SUCCESS;
}

}  // namespace dihip

using namespace dihip;

extern "C" {

int dihip_gemm_lowp_pack(void* stream, int wbits, const void* wq, const void* scales, const void* zeros, int N,
                         int K, int group_size, int dtype, void* w_packed, void* sz_packed) {
  DIHIP_REQUIRE(wbits == 4 || wbits == 8, DIHIP_PARAM_ERROR, "gemm_lowp_pack: wbits must be 4 or 8");
  DIHIP_REQUIRE(N > 0 && K > 0 && wq && scales && zeros && w_packed && sz_packed, DIHIP_PARAM_ERROR,
                "gemm_lowp_pack: bad argument");
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "gemm_lowp_pack: dtype");
  DIHIP_REQUIRE(group_size <= 0 || group_size % 32 == 0, DIHIP_PARAM_ERROR,
                "gemm_lowp_pack: GroupSize %d must be a multiple of 32", group_size);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const LowpDims d = lowp_dims(wbits, N, K, group_size);
  const size_t total = (size_t)d.NTILES * d.KT * 64 * 4;
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 65535);
  if (wbits == 4)
    hipLaunchKernelGGL(pack_w4_kernel, dim3(blocks), dim3(256), 0, s, (const uint8_t*)wq, (uint32_t*)w_packed, N, K,
                       d.KT, d.NTILES);
  else
    hipLaunchKernelGGL(pack_w8_kernel, dim3(blocks), dim3(256), 0, s, (const int8_t*)wq, (uint32_t*)w_packed, N, K,
                       d.KT, d.NTILES);
  const size_t sztotal = (size_t)d.Gp_packed * d.Np;
  hipLaunchKernelGGL(pack_sz_kernel, dim3((int)std::min<size_t>((sztotal + 255) / 256, 65535)), dim3(256), 0, s,
                     (const uint16_t*)scales, (const uint16_t*)zeros, (uint32_t*)sz_packed, N, d.Np, d.G, d.Gp_packed);
  return launch_status();
}

int dihip_dense_pack(void* stream, const void* w_kn, int N, int K, int dtype, void* w_packed) {
  DIHIP_REQUIRE(N > 0 && K > 0 && w_kn && w_packed, DIHIP_PARAM_ERROR, "dense_pack: bad argument");
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "dense_pack: dtype");
  const LowpDims d = lowp_dims(16, N, K, -1);
  const size_t total = (size_t)d.NTILES * d.KT * 64 * 4;
  hipLaunchKernelGGL(pack_w16_kernel, dim3((int)std::min<size_t>((total + 255) / 256, 65535)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (const uint16_t*)w_kn, (uint32_t*)w_packed, N, K, d.KT,
                     d.NTILES);
  return launch_status();
}

// What every entry point sets: activations x [M, K] with row stride K, one packed weight, alpha = 1.  The rest of the
// GemmCall (bias, residual, second weight, layouts, norm outputs ...) is the entry point's own.
static GemmCall make_call(int wbits, int dtype, int pro, int epi, const void* x, const void* w_packed, const void* sz_packed,
                          void* y, int M, int N, int K, int group_size, void* ws, size_t ws_bytes, void* sync) {
  GemmCall c{};
  c.wbits = wbits;
  c.dtype = dtype;
  c.pro = pro;
  c.epi = epi;
  c.x = x;
  c.ldx = K;
  c.w0 = w_packed;
  c.sz0 = sz_packed;
  c.y = y;
  c.M = M;
  c.N = N;
  c.K = K;
  c.group_size = group_size;
  c.alpha = 1.f;
  c.ws = ws;
  c.ws_bytes = ws_bytes;
  c.sync = sync;
  return c;
}

static int gemm_std(void* stream, int wbits, const void* x, const void* w, const void* sz, const void* bias,
                    const void* residual, void* y, int M, int N, int K, int group_size, int act, float alpha,
                    void* ws, size_t ws_bytes, void* sync, int dtype) {
  DIHIP_REQUIRE(y != nullptr || M == 0, DIHIP_PARAM_ERROR, "gemm_lowp: null output");
  GemmCall c = make_call(wbits, dtype, PRO_PLAIN, EPI_STD, x, w, sz, y, M, N, K, group_size, ws, ws_bytes, sync);
  c.bias = bias;
  c.residual = residual;
  c.act = act;
  c.alpha = alpha;
  return run_gemm(reinterpret_cast<hipStream_t>(stream), c);
}

int dihip_gemm_a16w8(void* stream, const void* x, const void* w_packed, const void* sz_packed, const void* bias,
                     const void* residual, void* y, int M, int N, int K, int group_size, int act, float alpha,
                     void* ws, size_t ws_bytes, void* sync, int dtype) {
  return gemm_std(stream, 8, x, w_packed, sz_packed, bias, residual, y, M, N, K, group_size, act, alpha, ws,
                  ws_bytes, sync, dtype);
}

int dihip_gemm_a16w4(void* stream, const void* x, const void* w_packed, const void* sz_packed, const void* bias,
                     const void* residual, void* y, int M, int N, int K, int group_size, int act, float alpha,
                     void* ws, size_t ws_bytes, void* sync, int dtype) {
  return gemm_std(stream, 4, x, w_packed, sz_packed, bias, residual, y, M, N, K, group_size, act, alpha, ws,
                  ws_bytes, sync, dtype);
}

// unquantised 16-bit weights (lm_head / dense Gemm), same kernel family
int dihip_gemm_a16w16(void* stream, const void* x, const void* w_packed, const void* bias, const void* residual,
                      void* y, int M, int N, int K, int act, float alpha, void* ws, size_t ws_bytes, void* sync,
                      int dtype) {
  GemmCall c = make_call(16, dtype, PRO_PLAIN, EPI_STD, x, w_packed, nullptr, y, M, N, K, -1, ws, ws_bytes, sync);
  c.bias = bias;
  c.residual = residual;
  c.act = act;
  c.alpha = alpha;
  return run_gemm(reinterpret_cast<hipStream_t>(stream), c);
}

// RMSNorm of M rows of the f32 hidden stream into FT rows (row-major or FRAG32)
static int launch_rmsnorm_rows(hipStream_t s, const float* h, const void* gamma, float eps, int M, int K, void* out, int frag_mt,
                               int dtype = DIHIP_BF16) {
  const bool vec = K % 4 == 0 && (reinterpret_cast<uintptr_t>(h) % 16 == 0) && (reinterpret_cast<uintptr_t>(gamma) % 8 == 0);
  uint16_t* xo = reinterpret_cast<uint16_t*>(out);
#define DIHIP_RMS_ROWS(FT_)                                                                                                        \
  do {                                                                                                                             \
    if (vec && K <= 4096)                                                                                                          \
      hipLaunchKernelGGL((rmsnorm_f32_to_ft_kernel<FT_, 4, 256>), dim3(M), dim3(256), 0, s, xo, h, gamma, eps, K, frag_mt);         \
    else if (vec && K <= 8192) /* wide rows: 1024 threads, two vectors each (256 threads took 6.8 us for 16 rows of 8192) */       \
      hipLaunchKernelGGL((rmsnorm_f32_to_ft_kernel<FT_, 2, 1024>), dim3(M), dim3(1024), 0, s, xo, h, gamma, eps, K, frag_mt);       \
    else                                                                                                                           \
      hipLaunchKernelGGL(rmsnorm_f32_to_ft_wide_kernel<FT_>, dim3(M), dim3(256), 0, s, xo, h, gamma, eps, K, frag_mt);              \
  } while (0)
  if (dtype == DIHIP_F16) DIHIP_RMS_ROWS(DIHIP_F16);
  else DIHIP_RMS_ROWS(DIHIP_BF16);
#undef DIHIP_RMS_ROWS
  return launch_status();
}

// The call's activations are RMSNorm(h; gamma, eps).  Up to GEMV_STREAM_MAX_M rows the norm is the decode GEMV's prologue.
// Beyond, it runs as its own small kernel into the tail of the call's workspace: the normalised rows are private to the
// call, so they are written in whatever layout the GEMM kernel that follows reads fastest (FRAG32 also when the output is).
static int set_norm_input(hipStream_t s, GemmCall& c, const float* h, const void* gamma, float eps) {
  if (c.M <= GEMV_STREAM_MAX_M) {
    c.pro = PRO_RMSNORM;
    c.x = h;
    c.gamma = gamma;
    c.eps = eps;
    return DIHIP_SUCCESS;
  }
  const bool dual = c.epi == EPI_SWIGLU;
  const size_t slab = lowp_slab_bytes(c.wbits, c.M, c.N, c.K, c.group_size, dual);
  const size_t off = (slab + 255) & ~(size_t)255;
  const bool frag = c.y_layout == DIHIP_ACT_FRAG32 || lowp_prefers_frag(c.wbits, c.M, c.N, c.K, c.group_size, dual);
  const int mt = c.M > 16 ? 2 : 1;
  const size_t xbytes = frag ? (size_t)mt * 16 * c.K * 2 : (size_t)c.M * c.K * 2;
  DIHIP_REQUIRE(c.ws && c.ws_bytes >= off + xbytes, DIHIP_MEMORY_ERROR, "fused gemm: workspace too small");
  void* xnorm = reinterpret_cast<char*>(c.ws) + off;
  c.x = xnorm;
  c.ws_bytes = off;
  c.x_layout = frag ? DIHIP_ACT_FRAG32 : DIHIP_ACT_ROWMAJOR;
  return launch_rmsnorm_rows(s, h, gamma, eps, c.M, c.K, xnorm, frag ? mt : 0, c.dtype);
}

int dihip_fused_norm_gemm(void* stream, int wbits, const float* h, const void* gamma, float eps, const void* w_packed,
                          const void* sz_packed, const void* bias, void* y, int M, int N, int K, int group_size,
                          int act, void* ws, size_t ws_bytes, void* sync, int dtype) {
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "fused path: bf16 or f16 activations");
  DIHIP_REQUIRE(sync != nullptr, DIHIP_PARAM_ERROR, "fused path needs a sync buffer");
  if (M == 0) return DIHIP_SUCCESS;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GemmCall c = make_call(wbits, dtype, PRO_PLAIN, EPI_STD, nullptr, w_packed, sz_packed, y, M, N, K, group_size, ws, ws_bytes, sync);
  c.bias = bias;
  c.act = act;
  if (int st = set_norm_input(s, c, h, gamma, eps)) return st;
  return run_gemm(s, c);
}

int dihip_fused_norm_swiglu(void* stream, int wbits, const float* h, const void* gamma, float eps,
                            const void* wg_packed, const void* szg_packed, const void* wu_packed,
                            const void* szu_packed, void* y, int M, int N, int K, int group_size, void* ws,
                            size_t ws_bytes, void* sync, int dtype) {
  return dihip_fused_norm_swiglu_ex(stream, wbits, h, gamma, eps, wg_packed, szg_packed, wu_packed, szu_packed, y, M, N, K,
                                    group_size, ws, ws_bytes, sync, dtype, DIHIP_ACT_ROWMAJOR);
}

int dihip_fused_norm_swiglu_ex(void* stream, int wbits, const float* h, const void* gamma, float eps,
                               const void* wg_packed, const void* szg_packed, const void* wu_packed,
                               const void* szu_packed, void* y, int M, int N, int K, int group_size, void* ws,
                               size_t ws_bytes, void* sync, int dtype, int y_layout) {
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "fused path: bf16 or f16 activations");
  DIHIP_REQUIRE(y_layout == DIHIP_ACT_ROWMAJOR || y_layout == DIHIP_ACT_FRAG32, DIHIP_PARAM_ERROR, "fused swiglu: bad y_layout");
  DIHIP_REQUIRE(y_layout == DIHIP_ACT_ROWMAJOR || (M > GEMV_STREAM_MAX_M && lowp_frag_served(wbits, dtype, M, N, K, group_size, true)),
                DIHIP_PARAM_ERROR, "fused swiglu: FRAG32 output needs the small-batch kernel (4 < M <= 32, K a multiple of the k-tile)");
  DIHIP_REQUIRE(sync != nullptr, DIHIP_PARAM_ERROR, "fused path needs a sync buffer");
  if (M == 0) return DIHIP_SUCCESS;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GemmCall c = make_call(wbits, dtype, PRO_PLAIN, EPI_SWIGLU, nullptr, wg_packed, szg_packed, y, M, N, K, group_size, ws, ws_bytes, sync);
  c.w1 = wu_packed;
  c.sz1 = szu_packed;
  c.y_layout = y_layout;
  if (int st = set_norm_input(s, c, h, gamma, eps)) return st;
  return run_gemm(s, c);
}

int dihip_lm_head(void* stream, float* logits, const float* h, const void* gamma, float eps, const void* w_packed,
                  int M, int N, int K, void* ws, size_t ws_bytes, void* sync, int dtype) {
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "lm_head: dtype");
  DIHIP_REQUIRE(logits && h && w_packed && sync, DIHIP_PARAM_ERROR, "lm_head: null pointer");
  if (M == 0) return DIHIP_SUCCESS;
  DIHIP_REQUIRE(gamma != nullptr, DIHIP_PARAM_ERROR, "lm_head: needs gamma");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GemmCall c = make_call(16, dtype, PRO_PLAIN, EPI_ADDTO, nullptr, w_packed, nullptr, nullptr, M, N, K, -1, ws, ws_bytes, sync);
  c.h_out = logits;
  if (int st = set_norm_input(s, c, h, gamma, eps)) return st;
  return run_gemm(s, c);
}

int dihip_fused_gemm_addto(void* stream, int wbits, const void* x, const void* w_packed, const void* sz_packed,
                           const float* h_res, float* h_out, int M, int N, int K, int group_size, void* ws,
                           size_t ws_bytes, void* sync, int dtype) {
  return dihip_fused_gemm_addto_ex(stream, wbits, x, w_packed, sz_packed, h_res, h_out, M, N, K, group_size, ws, ws_bytes,
                                   sync, dtype, DIHIP_ACT_ROWMAJOR);
}

size_t dihip_act_frag_bytes(int M, int K) {
  if (M <= 0 || M > 32 || K <= 0 || K % 32) return 0;
  return (size_t)(M > 16 ? 32 : 16) * K * 2;
}

static int act_convert(void* stream, const void* src, void* dst, int M, int K, int dtype, int to_frag) {
  DIHIP_REQUIRE(src && dst && M > 0 && M <= 32 && K > 0 && K % 32 == 0, DIHIP_PARAM_ERROR,
                "act_frag: need 0 < M <= 32 and K a multiple of 32");
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "act_frag: 16-bit activations only");
  const size_t total = (size_t)M * K;
  hipLaunchKernelGGL(act_frag_convert_kernel, dim3((int)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (uint16_t*)dst, (const uint16_t*)src, M, K, M > 16 ? 2 : 1, to_frag);
  return launch_status();
}
int dihip_act_to_frag(void* stream, const void* x_rowmajor, void* x_frag, int M, int K, int dtype) {
  return act_convert(stream, x_rowmajor, x_frag, M, K, dtype, 1);
}
int dihip_act_from_frag(void* stream, const void* x_frag, void* x_rowmajor, int M, int K, int dtype) {
  return act_convert(stream, x_frag, x_rowmajor, M, K, dtype, 0);
}

int dihip_fused_gemm_addto_ex(void* stream, int wbits, const void* x, const void* w_packed, const void* sz_packed,
                              const float* h_res, float* h_out, int M, int N, int K, int group_size, void* ws,
                              size_t ws_bytes, void* sync, int dtype, int x_layout) {
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "fused path: bf16 or f16 activations");
  DIHIP_REQUIRE(x_layout == DIHIP_ACT_ROWMAJOR || x_layout == DIHIP_ACT_FRAG32, DIHIP_PARAM_ERROR, "fused addto: bad x_layout");
  // h_res may be NULL: then h_out = x . W (row-parallel TP ranks other than 0, gemm_op.cpp:133-137)
  DIHIP_REQUIRE(sync != nullptr && h_out, DIHIP_PARAM_ERROR, "fused addto: null pointer");
  GemmCall c = make_call(wbits, dtype, PRO_PLAIN, EPI_ADDTO, x, w_packed, sz_packed, nullptr, M, N, K, group_size, ws, ws_bytes, sync);
  c.x_layout = x_layout;
  c.h_res = h_res;
  c.h_out = h_out;
  return run_gemm(reinterpret_cast<hipStream_t>(stream), c);
}

static int gemm_addto_norm_impl(void* stream, int wbits, const void* x, const void* w_packed, const void* sz_packed,
                                const float* h_res, float* h_out, int M, int N, int K, int group_size, void* ws,
                                size_t ws_bytes, void* sync, int dtype, int x_layout, const void* gamma, float eps,
                                void* xnorm, int xnorm_layout, float* rowsq, size_t rowsq_bytes, int* rowsq_parts) {
  if (rowsq_parts) *rowsq_parts = 0;
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "fused path: bf16 or f16 activations");
  DIHIP_REQUIRE(x_layout == DIHIP_ACT_ROWMAJOR || x_layout == DIHIP_ACT_FRAG32, DIHIP_PARAM_ERROR, "fused addto: bad x_layout");
  DIHIP_REQUIRE(xnorm_layout == DIHIP_ACT_ROWMAJOR || (xnorm_layout == DIHIP_ACT_FRAG32 && M <= 32 && N % 32 == 0),
                DIHIP_PARAM_ERROR, "fused addto + norm: FRAG32 output needs M <= 32 and N %% 32 == 0");
  DIHIP_REQUIRE(sync != nullptr && h_out && gamma && xnorm, DIHIP_PARAM_ERROR, "fused addto + norm: null pointer");
  if (M == 0) return DIHIP_SUCCESS;
  bool done = false;
  GemmCall c = make_call(wbits, dtype, PRO_PLAIN, EPI_ADDTO, x, w_packed, sz_packed, nullptr, M, N, K, group_size, ws, ws_bytes, sync);
  c.x_layout = x_layout;
  c.h_res = h_res;
  c.h_out = h_out;
  c.n_gamma = gamma;
  c.n_eps = eps;
  c.n_out = xnorm;
  c.n_frag_mt = xnorm_layout == DIHIP_ACT_FRAG32 ? (M > 16 ? 2 : 1) : 0;
  c.n_done = &done;
  c.n_rowsq = rowsq;
  c.n_rowsq_bytes = rowsq_bytes;
  c.n_parts = rowsq ? rowsq_parts : nullptr;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int st = run_gemm(s, c);
  if (st || done) return st;
  return launch_rmsnorm_rows(s, h_out, gamma, eps, M, N, xnorm, c.n_frag_mt, dtype);  // this plan has no slab reduction to ride on
}

int dihip_fused_gemm_addto_norm(void* stream, int wbits, const void* x, const void* w_packed, const void* sz_packed,
                                const float* h_res, float* h_out, int M, int N, int K, int group_size, void* ws,
                                size_t ws_bytes, void* sync, int dtype, int x_layout, const void* gamma, float eps,
                                void* xnorm, int xnorm_layout) {
  return gemm_addto_norm_impl(stream, wbits, x, w_packed, sz_packed, h_res, h_out, M, N, K, group_size, ws, ws_bytes, sync, dtype, x_layout,
                              gamma, eps, xnorm, xnorm_layout, nullptr, 0, nullptr);
}

// ... with the RMSNorm DEFERRED where the serving kernel offers it (gemv_batch_kernel.hpp): *rowsq_parts > 0 -- xnorm holds
// FT(gamma * h_out) and rowsq[part][32] the partial sums of h_out^2, to be handed to dihip_prenorm_{gemm,swiglu}_rowsq;
// *rowsq_parts == 0 -- xnorm is the finished norm (as dihip_fused_gemm_addto_norm)
int dihip_fused_gemm_addto_prenorm(void* stream, int wbits, const void* x, const void* w_packed, const void* sz_packed,
                                   const float* h_res, float* h_out, int M, int N, int K, int group_size, void* ws,
                                   size_t ws_bytes, void* sync, int dtype, int x_layout, const void* gamma, float eps,
                                   void* xnorm, int xnorm_layout, float* rowsq, size_t rowsq_bytes, int* rowsq_parts) {
  DIHIP_REQUIRE(rowsq && rowsq_parts && reinterpret_cast<uintptr_t>(rowsq) % 16 == 0, DIHIP_PARAM_ERROR, "fused addto + prenorm: null / misaligned rowsq");
  return gemm_addto_norm_impl(stream, wbits, x, w_packed, sz_packed, h_res, h_out, M, N, K, group_size, ws, ws_bytes, sync, dtype, x_layout,
                              gamma, eps, xnorm, xnorm_layout, rowsq, rowsq_bytes, rowsq_parts);
}

size_t dihip_rowsq_bytes() { return (size_t)256 * 32 * sizeof(float); }  // one part per workgroup of a producer (<= one per CU)

// LayerNormNoBeta of the f32 hidden rows into FT rows, on its own (the MoE layer feeds four consumers from it)
int dihip_rmsnorm_rows(void* stream, void* xnorm, const float* h, const void* gamma, float eps, int M, int K, int dtype) {
  DIHIP_REQUIRE(M >= 0 && K > 0 && xnorm && h && gamma, DIHIP_PARAM_ERROR, "rmsnorm_rows: bad argument");
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "rmsnorm_rows: 16-bit rows only");
  if (M == 0) return DIHIP_SUCCESS;
  return launch_rmsnorm_rows(reinterpret_cast<hipStream_t>(stream), h, gamma, eps, M, K, xnorm, 0, dtype);
}

int dihip_prenorm_gemm(void* stream, int wbits, const void* xnorm, int x_layout, const void* w_packed, const void* sz_packed,
                       const void* bias, void* y, int M, int N, int K, int group_size, int act, void* ws, size_t ws_bytes,
                       void* sync, int dtype) {
  return dihip_prenorm_gemm_rowsq(stream, wbits, xnorm, x_layout, w_packed, sz_packed, bias, y, M, N, K, group_size, act, ws, ws_bytes, sync,
                                  dtype, nullptr, 0, 0.f);
}

// the activations of a prenorm call: normalised rows in either layout, with or without deferred row norms
static void set_prenorm_input(GemmCall& c, int x_layout, const float* rowsq, int rowsq_parts, float eps) {
  c.x_layout = x_layout;
  c.rowsq = rowsq_parts > 0 ? rowsq : nullptr;
  c.rowsq_parts = rowsq_parts;
  c.rowsq_eps = eps;
}

int dihip_prenorm_gemm_rowsq(void* stream, int wbits, const void* xnorm, int x_layout, const void* w_packed, const void* sz_packed,
                             const void* bias, void* y, int M, int N, int K, int group_size, int act, void* ws, size_t ws_bytes,
                             void* sync, int dtype, const float* rowsq, int rowsq_parts, float eps) {
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "fused path: bf16 or f16 activations");
  DIHIP_REQUIRE(x_layout == DIHIP_ACT_ROWMAJOR || x_layout == DIHIP_ACT_FRAG32, DIHIP_PARAM_ERROR, "prenorm gemm: bad x_layout");
  DIHIP_REQUIRE(sync != nullptr && xnorm && y, DIHIP_PARAM_ERROR, "prenorm gemm: null pointer");
  GemmCall c = make_call(wbits, dtype, PRO_PLAIN, EPI_STD, xnorm, w_packed, sz_packed, y, M, N, K, group_size, ws, ws_bytes, sync);
  c.bias = bias;
  c.act = act;
  set_prenorm_input(c, x_layout, rowsq, rowsq_parts, eps);
  return run_gemm(reinterpret_cast<hipStream_t>(stream), c);
}

int dihip_prenorm_swiglu(void* stream, int wbits, const void* xnorm, int x_layout, const void* wg_packed,
                         const void* szg_packed, const void* wu_packed, const void* szu_packed, void* y, int M, int N, int K,
                         int group_size, void* ws, size_t ws_bytes, void* sync, int dtype, int y_layout) {
  return dihip_prenorm_swiglu_rowsq(stream, wbits, xnorm, x_layout, wg_packed, szg_packed, wu_packed, szu_packed, y, M, N, K, group_size, ws,
                                    ws_bytes, sync, dtype, y_layout, nullptr, 0, 0.f);
}

int dihip_prenorm_swiglu_rowsq(void* stream, int wbits, const void* xnorm, int x_layout, const void* wg_packed,
                               const void* szg_packed, const void* wu_packed, const void* szu_packed, void* y, int M, int N, int K,
                               int group_size, void* ws, size_t ws_bytes, void* sync, int dtype, int y_layout, const float* rowsq,
                               int rowsq_parts, float eps) {
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "fused path: bf16 or f16 activations");
  DIHIP_REQUIRE(x_layout == DIHIP_ACT_ROWMAJOR || x_layout == DIHIP_ACT_FRAG32, DIHIP_PARAM_ERROR, "prenorm swiglu: bad x_layout");
  DIHIP_REQUIRE(y_layout == DIHIP_ACT_ROWMAJOR || y_layout == DIHIP_ACT_FRAG32, DIHIP_PARAM_ERROR, "prenorm swiglu: bad y_layout");
  DIHIP_REQUIRE(sync != nullptr && xnorm && y, DIHIP_PARAM_ERROR, "prenorm swiglu: null pointer");
  DIHIP_REQUIRE(y_layout == DIHIP_ACT_ROWMAJOR || (M > GEMV_STREAM_MAX_M && lowp_frag_served(wbits, dtype, M, N, K, group_size, true)),
                DIHIP_PARAM_ERROR, "prenorm swiglu: FRAG32 output needs the small-batch kernel (4 < M <= 32, K a multiple of the k-tile)");
  GemmCall c = make_call(wbits, dtype, PRO_PLAIN, EPI_SWIGLU, xnorm, wg_packed, szg_packed, y, M, N, K, group_size, ws, ws_bytes, sync);
  c.w1 = wu_packed;
  c.sz1 = szu_packed;
  c.y_layout = y_layout;
  set_prenorm_input(c, x_layout, rowsq, rowsq_parts, eps);
  return run_gemm(reinterpret_cast<hipStream_t>(stream), c);
}

}  // extern "C"
