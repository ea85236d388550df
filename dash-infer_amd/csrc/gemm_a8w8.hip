// gemm_a8w8.hip -- activation quantiser and C-ABI entry points of the int8-activation GEMM
// (include/dashinfer_hip.h section 1c; kernel: gemm_a8w8_kernel.hpp).
#include <algorithm>

#include "gemm_a8w8_kernel.hpp"

namespace dihip {

// ------------------------------------------------------------------------------------------
// Per-row symmetric dynamic quantisation (replaces per_channel_symm_dynamic_quantization,
// gemm_a8w8_perc_kernel.cu:28-133), every line one IEEE f32 operation:
//   amax = max_k |x|;  a_scale = amax / 127;  rec = 127 / amax;  q = int8(rint(min(127, max(-128, x * rec))));  rsum = sum_k q
// a row of zeros: q = 0, a_scale = 0.  One workgroup per row; thread t owns the 4-element vectors t, t + THREADS, ...; with
// VPT > 0 the row stays in registers between the max and the rounding (one pass over memory, no atomics); VPT == 0 reads it a
// second time (rows wider than THREADS * 4 * VPT: they come back from the caches).  The int8 row is written out to Kp = the
// row padded to the 64-wide k-tile, zeros beyond K (the GEMM's B padding is -128 there).
// NORM: the row is FT(RMSNorm(h) * gamma) of an f32 hidden row, with the arithmetic, the thread mapping and the summation
// order of rmsnorm_f32_to_ft_kernel<FT, VPT, THREADS> (gemm_lowp.hip) -- the values dihip_rmsnorm_rows writes, rounded to FT
// BEFORE they are quantised, as the reference's LayerNormNoBeta -> GemmA8W8 pair does.
// ------------------------------------------------------------------------------------------
template <int FT, bool NORM, int VPT, int THREADS>
__global__ __launch_bounds__(THREADS) void act_quant_i8_kernel(const void* __restrict__ x, int ldx, const void* __restrict__ gamma,
                                                                float eps, int K, int Kp, int vec_ok, int8_t* __restrict__ xq,
                                                                float* __restrict__ a_scale, int* __restrict__ rsum) {
  constexpr int NW = THREADS / 64;
  __shared__ float redf[NW];
  __shared__ float redm[NW];
  __shared__ int redi[NW];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int nvec = Kp >> 2;  // vectors of the padded row
  float rstd = 0.f;
  f32x4_t hv[NORM && VPT ? VPT : 1];
  if constexpr (NORM) {
    static_assert(VPT > 0, "the norm form holds the row");
    const f32x4_t* hr = reinterpret_cast<const f32x4_t*>(reinterpret_cast<const float*>(x) + (size_t)row * K);
    const int nv = K >> 2;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int c = tid + i * THREADS;
      hv[i] = c < nv ? hr[c] : f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) ss += (hv[i][0] * hv[i][0] + hv[i][1] * hv[i][1]) + (hv[i][2] * hv[i][2] + hv[i][3] * hv[i][3]);
    ss = wave_sum(ss);
    if ((tid & 63) == 0) redf[tid >> 6] = ss;
    __syncthreads();
    float tot = redf[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) tot += redf[w];
    rstd = 1.f / sqrtf(tot / (float)K + eps);
  }
  // the 4 values of vector c (0 beyond K)
  auto fetch = [&](int c, int i) -> f32x4_t {
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    const int k = c * 4;
    if constexpr (NORM) {
      if (k < K) {  // K % 4 == 0
        const u32x2_t gm = reinterpret_cast<const u32x2_t*>(gamma)[c];
        const float g0 = ft_bits_to_f32<FT>(gm[0] & 0xFFFFu), g1 = ft_bits_to_f32<FT>(gm[0] >> 16);
        const float g2 = ft_bits_to_f32<FT>(gm[1] & 0xFFFFu), g3 = ft_bits_to_f32<FT>(gm[1] >> 16);
        v[0] = ft_round<FT>((g0 * hv[i][0]) * rstd);
        v[1] = ft_round<FT>((g1 * hv[i][1]) * rstd);
        v[2] = ft_round<FT>((g2 * hv[i][2]) * rstd);
        v[3] = ft_round<FT>((g3 * hv[i][3]) * rstd);
      }
    } else {
      const uint16_t* xr = reinterpret_cast<const uint16_t*>(x) + (size_t)row * ldx;
      if (vec_ok && k + 3 < K) {
        const u32x2_t d = *reinterpret_cast<const u32x2_t*>(xr + k);
        v[0] = ft_bits_to_f32<FT>(d[0] & 0xFFFFu);
        v[1] = ft_bits_to_f32<FT>(d[0] >> 16);
        v[2] = ft_bits_to_f32<FT>(d[1] & 0xFFFFu);
        v[3] = ft_bits_to_f32<FT>(d[1] >> 16);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < K) v[j] = ft_bits_to_f32<FT>(xr[k + j]);
      }
    }
    return v;
  };

  constexpr int HOLD = VPT ? VPT : 1;
  f32x4_t xv[HOLD];
  float amax = 0.f;
  if constexpr (VPT > 0) {
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int c = tid + i * THREADS;
      xv[i] = c < nvec ? fetch(c, i) : f32x4_t{0.f, 0.f, 0.f, 0.f};
      amax = fmaxf(amax, fmaxf(fmaxf(fabsf(xv[i][0]), fabsf(xv[i][1])), fmaxf(fabsf(xv[i][2]), fabsf(xv[i][3]))));
    }
  } else {
    for (int c = tid; c < nvec; c += THREADS) {
      const f32x4_t v = fetch(c, 0);
      amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
  }
  amax = wave_max(amax);
  if ((tid & 63) == 0) redm[tid >> 6] = amax;
  __syncthreads();
  amax = redm[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) amax = fmaxf(amax, redm[w]);
  const float scale = amax / 127.f;
  const float rec = amax > 0.f ? 127.f / amax : 0.f;

  int* qrow = reinterpret_cast<int*>(xq + (size_t)row * Kp);
  int sum = 0;
  auto quant = [&](const f32x4_t& v, int c) {
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = (int)rintf(fminf(127.f, fmaxf(-128.f, v[j] * rec)));
      sum += q;
      d |= (uint32_t)(q & 0xFF) << (8 * j);
    }
    qrow[c] = (int)d;
  };
  if constexpr (VPT > 0) {
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int c = tid + i * THREADS;
      if (c < nvec) quant(xv[i], c);
    }
  } else {
    for (int c = tid; c < nvec; c += THREADS) quant(fetch(c, 0), c);
  }
  // |sum| <= 128 * K: exact in i32
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((tid & 63) == 0) redi[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    int tot = redi[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) tot += redi[w];
    rsum[row] = tot;
    a_scale[row] = scale;
  }
}

constexpr int A8W8_MAX_K = 131072;  // 127 * 128 * K < 2^31

static inline int a8_roundup(int v, int m) { return (v + m - 1) / m * m; }
static inline size_t a8_align(size_t v) { return (v + 255) & ~(size_t)255; }

struct A8Workspace {
  size_t xq_off, scale_off, rsum_off, norm_off, total;
};
static A8Workspace a8_workspace(int M, int K) {
  A8Workspace w{};
  const size_t Kp = (size_t)a8_roundup(K, 64);
  w.xq_off = 0;
  w.scale_off = a8_align((size_t)M * Kp);
  w.rsum_off = w.scale_off + a8_align((size_t)M * sizeof(float));
  w.norm_off = w.rsum_off + a8_align((size_t)M * sizeof(int));
  w.total = w.norm_off + a8_align((size_t)M * K * 2);  // FT rows of the two-launch norm form (rows the one-launch form does not take)
  return w;
}

static int run_act_quant(hipStream_t s, const void* x, int ldx, int M, int K, int dtype, void* xq, float* a_scale, int* rsum) {
  DIHIP_REQUIRE(M >= 0 && K > 0 && K <= A8W8_MAX_K && ldx >= K, DIHIP_PARAM_ERROR,
                "act_quant_i8: bad shape M=%d K=%d ldx=%d (K <= %d: the int32 products must not overflow)", M, K, ldx, A8W8_MAX_K);
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "act_quant_i8: activation type must be FLOAT16 or BFLOAT16");
  if (M == 0) return DIHIP_SUCCESS;
  DIHIP_REQUIRE(x && xq && a_scale && rsum, DIHIP_PARAM_ERROR, "act_quant_i8: null pointer");
  DIHIP_REQUIRE(reinterpret_cast<uintptr_t>(xq) % 16 == 0, DIHIP_PARAM_ERROR, "act_quant_i8: xq must be 16-byte aligned");
  const int Kp = a8_roundup(K, 64);
  const int vec_ok = (ldx % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 8 == 0);
  int8_t* q = reinterpret_cast<int8_t*>(xq);
#define DIHIP_AQ(FT_, VPT_)                                                                                                  \
  hipLaunchKernelGGL((act_quant_i8_kernel<FT_, false, VPT_, 256>), dim3(M), dim3(256), 0, s, x, ldx, nullptr, 0.f, K, Kp, vec_ok, q, \
                     a_scale, rsum)
#define DIHIP_AQ_ALL(FT_)                           \
  do {                                              \
    if (Kp <= 256 * 4 * 4) DIHIP_AQ(FT_, 4);        \
    else if (Kp <= 256 * 4 * 8) DIHIP_AQ(FT_, 8);   \
    else if (Kp <= 256 * 4 * 20) DIHIP_AQ(FT_, 20); \
    else DIHIP_AQ(FT_, 0);                          \
  } while (0)
  if (dtype == DIHIP_F16) DIHIP_AQ_ALL(DIHIP_F16);
  else DIHIP_AQ_ALL(DIHIP_BF16);
#undef DIHIP_AQ_ALL
#undef DIHIP_AQ
  return launch_status();
}

// one launch when rmsnorm_f32_to_ft_kernel would serve the row (same mapping, same sums); otherwise dihip_rmsnorm_rows into
// `tmp` (FT [M, K]) and the plain quantiser
static int run_norm_act_quant(hipStream_t s, const float* h, const void* gamma, float eps, int M, int K, int dtype, void* xq,
                              float* a_scale, int* rsum, void* tmp, size_t tmp_bytes) {
  DIHIP_REQUIRE(M >= 0 && K > 0 && K <= A8W8_MAX_K, DIHIP_PARAM_ERROR, "norm_act_quant_i8: bad shape M=%d K=%d", M, K);
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "norm_act_quant_i8: activation type must be FLOAT16 or BFLOAT16");
  if (M == 0) return DIHIP_SUCCESS;
  DIHIP_REQUIRE(h && gamma && xq && a_scale && rsum, DIHIP_PARAM_ERROR, "norm_act_quant_i8: null pointer");
  DIHIP_REQUIRE(reinterpret_cast<uintptr_t>(xq) % 16 == 0, DIHIP_PARAM_ERROR, "norm_act_quant_i8: xq must be 16-byte aligned");
  const int Kp = a8_roundup(K, 64);
  const bool vec = K % 4 == 0 && (reinterpret_cast<uintptr_t>(h) % 16 == 0) && (reinterpret_cast<uintptr_t>(gamma) % 8 == 0);
  int8_t* q = reinterpret_cast<int8_t*>(xq);
  // (the padded row must fit the held vectors too: Kp <= THREADS * 4 * VPT)
  if (vec && K <= 4096) {
    if (dtype == DIHIP_F16)
      hipLaunchKernelGGL((act_quant_i8_kernel<DIHIP_F16, true, 4, 256>), dim3(M), dim3(256), 0, s, h, K, gamma, eps, K, Kp, 1, q, a_scale, rsum);
    else
      hipLaunchKernelGGL((act_quant_i8_kernel<DIHIP_BF16, true, 4, 256>), dim3(M), dim3(256), 0, s, h, K, gamma, eps, K, Kp, 1, q, a_scale, rsum);
    return launch_status();
  }
  if (vec && K <= 8192) {
    if (dtype == DIHIP_F16)
      hipLaunchKernelGGL((act_quant_i8_kernel<DIHIP_F16, true, 2, 1024>), dim3(M), dim3(1024), 0, s, h, K, gamma, eps, K, Kp, 1, q, a_scale, rsum);
    else
      hipLaunchKernelGGL((act_quant_i8_kernel<DIHIP_BF16, true, 2, 1024>), dim3(M), dim3(1024), 0, s, h, K, gamma, eps, K, Kp, 1, q, a_scale, rsum);
    return launch_status();
  }
  DIHIP_REQUIRE(tmp && tmp_bytes >= (size_t)M * K * 2 && reinterpret_cast<uintptr_t>(tmp) % 16 == 0, DIHIP_MEMORY_ERROR,
                "norm_act_quant_i8: rows of K=%d need %zu bytes of workspace for the normalised rows", K, (size_t)M * K * 2);
  const int st = dihip_rmsnorm_rows(s, tmp, h, gamma, eps, M, K, dtype);
  if (st) return st;
  return run_act_quant(s, tmp, K, M, K, dtype, xq, a_scale, rsum);
}

static int run_gemm_a8w8(hipStream_t s, int epi, const void* xq, const float* a_scale, const int* rsum, const void* w0, const void* sz0,
                         const void* w1, const void* sz1, const void* bias, const void* residual, void* y, const float* h_res,
                         float* h_out, int M, int N, int K, int act, int dtype) {
  DIHIP_REQUIRE(M >= 0 && N > 0 && K > 0, DIHIP_PARAM_ERROR, "gemm_a8w8: bad shape M=%d N=%d K=%d", M, N, K);
  DIHIP_REQUIRE(K <= A8W8_MAX_K, DIHIP_PARAM_ERROR, "gemm_a8w8: K = %d exceeds %d (the int32 accumulator would overflow)", K, A8W8_MAX_K);
  DIHIP_REQUIRE(dtype == DIHIP_BF16 || dtype == DIHIP_F16, DIHIP_PARAM_ERROR, "gemm_a8w8: output type must be FLOAT16 or BFLOAT16");
  DIHIP_REQUIRE(act >= DIHIP_ACT_NONE && act <= DIHIP_ACT_SIGMOID, DIHIP_PARAM_ERROR, "gemm_a8w8: unknown activation %d", act);
  if (M == 0) return DIHIP_SUCCESS;
  const bool dual = epi == EPI_SWIGLU;
  DIHIP_REQUIRE(xq && a_scale && rsum && w0 && sz0 && (!dual || (w1 && sz1)), DIHIP_PARAM_ERROR, "gemm_a8w8: null input pointer");
  DIHIP_REQUIRE(epi == EPI_ADDTO ? h_out != nullptr : y != nullptr, DIHIP_PARAM_ERROR, "gemm_a8w8: null output");
  DIHIP_REQUIRE(reinterpret_cast<uintptr_t>(xq) % 8 == 0, DIHIP_PARAM_ERROR, "gemm_a8w8: xq must be 8-byte aligned");
  A8Args a{};
  a.w0 = reinterpret_cast<const u32x4_t*>(w0);
  a.w1 = reinterpret_cast<const u32x4_t*>(w1);
  a.sz0 = reinterpret_cast<const uint32_t*>(sz0);
  a.sz1 = reinterpret_cast<const uint32_t*>(sz1);
  a.xq = reinterpret_cast<const int8_t*>(xq);
  a.KT = a8_roundup(K, 64) / 64;
  a.ldq = a.KT * 64;
  a.a_scale = a_scale;
  a.rsum = rsum;
  a.bias = bias;
  a.residual = residual;
  a.y = y;
  a.h_res = h_res;
  a.h_out = h_out;
  a.act = act;
  a.M = M;
  a.N = N;
  a.NTILES = (N + 15) / 16;
  const int tiles_per_block = dual ? A8_WAVES * A8_CW / 2 : A8_WAVES * A8_CW;
  const int col_blocks = (a.NTILES + tiles_per_block - 1) / tiles_per_block;
  const int blocks = col_blocks * ((M + A8_BM - 1) / A8_BM);
  hipError_t e = hipErrorInvalidValue;
#define A8_GO(EPI_) \
  if (epi == EPI_) e = dtype == DIHIP_F16 ? launch_gemm_a8w8<DIHIP_F16, EPI_>(a, blocks, s) : launch_gemm_a8w8<DIHIP_BF16, EPI_>(a, blocks, s);
  A8_GO(EPI_STD) A8_GO(EPI_SWIGLU) A8_GO(EPI_ADDTO)
#undef A8_GO
  DIHIP_REQUIRE(e == hipSuccess, DIHIP_RUNTIME_ERROR, "gemm_a8w8: launch failed (M=%d N=%d K=%d epi=%d): %s", M, N, K, epi, hipGetErrorString(e));
  return DIHIP_SUCCESS;
}

// the quantised row, its scale and its sum inside a caller's workspace
struct A8Slices {
  void* xq;
  float* a_scale;
  int* rsum;
  void* tmp;
  size_t tmp_bytes;
};
static int a8_slices(void* ws, size_t ws_bytes, int M, int K, A8Slices* o) {
  DIHIP_REQUIRE(M >= 0 && K > 0 && K <= A8W8_MAX_K, DIHIP_PARAM_ERROR, "gemm_a8w8: bad shape M=%d K=%d (K <= %d)", M, K, A8W8_MAX_K);
  const A8Workspace w = a8_workspace(M, K);
  DIHIP_REQUIRE(M == 0 || (ws && ws_bytes >= w.norm_off && reinterpret_cast<uintptr_t>(ws) % 16 == 0), DIHIP_MEMORY_ERROR,
                "gemm_a8w8: workspace too small or misaligned (%zu < %zu); see dihip_gemm_a8w8_workspace_bytes", ws_bytes, w.norm_off);
  char* p = reinterpret_cast<char*>(ws);
  o->xq = p + w.xq_off;
  o->a_scale = reinterpret_cast<float*>(p + w.scale_off);
  o->rsum = reinterpret_cast<int*>(p + w.rsum_off);
  o->tmp = ws_bytes > w.norm_off ? p + w.norm_off : nullptr;
  o->tmp_bytes = ws_bytes > w.norm_off ? ws_bytes - w.norm_off : 0;
  return DIHIP_SUCCESS;
}

}  // namespace dihip

using namespace dihip;

extern "C" {

size_t dihip_gemm_a8w8_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0 || K > A8W8_MAX_K) return 0;
  return a8_workspace(M, K).total;
}

int dihip_act_quant_i8(void* stream, const void* x, int ldx, int M, int K, int dtype, void* xq, float* a_scale, int* rsum) {
  return run_act_quant(reinterpret_cast<hipStream_t>(stream), x, ldx, M, K, dtype, xq, a_scale, rsum);
}

int dihip_norm_act_quant_i8(void* stream, const float* h, const void* gamma, float eps, int M, int K, int dtype, void* xq,
                            float* a_scale, int* rsum, void* ws, size_t ws_bytes) {
  return run_norm_act_quant(reinterpret_cast<hipStream_t>(stream), h, gamma, eps, M, K, dtype, xq, a_scale, rsum, ws, ws_bytes);
}

int dihip_gemm_a8w8_q(void* stream, const void* xq, const float* a_scale, const int* rsum, const void* w_packed, const void* sz_packed,
                      const void* bias, const void* residual, void* y, int M, int N, int K, int act, int dtype) {
  return run_gemm_a8w8(reinterpret_cast<hipStream_t>(stream), EPI_STD, xq, a_scale, rsum, w_packed, sz_packed, nullptr, nullptr, bias,
                       residual, y, nullptr, nullptr, M, N, K, act, dtype);
}

int dihip_gemm_a8w8_swiglu_q(void* stream, const void* xq, const float* a_scale, const int* rsum, const void* wg_packed,
                             const void* szg_packed, const void* wu_packed, const void* szu_packed, void* y, int M, int N, int K,
                             int dtype) {
  return run_gemm_a8w8(reinterpret_cast<hipStream_t>(stream), EPI_SWIGLU, xq, a_scale, rsum, wg_packed, szg_packed, wu_packed,
                       szu_packed, nullptr, nullptr, y, nullptr, nullptr, M, N, K, DIHIP_ACT_NONE, dtype);
}

int dihip_gemm_a8w8_addto_q(void* stream, const void* xq, const float* a_scale, const int* rsum, const void* w_packed,
                            const void* sz_packed, const float* h_res, float* h_out, int M, int N, int K, int dtype) {
  return run_gemm_a8w8(reinterpret_cast<hipStream_t>(stream), EPI_ADDTO, xq, a_scale, rsum, w_packed, sz_packed, nullptr, nullptr,
                       nullptr, nullptr, nullptr, h_res, h_out, M, N, K, DIHIP_ACT_NONE, dtype);
}

int dihip_gemm_a8w8(void* stream, const void* x, const void* w_packed, const void* sz_packed, const void* bias, const void* residual,
                    void* y, int M, int N, int K, int act, void* ws, size_t ws_bytes, int dtype) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  A8Slices q;
  int st = a8_slices(ws, ws_bytes, M, K, &q);
  if (st) return st;
  if ((st = run_act_quant(s, x, K, M, K, dtype, q.xq, q.a_scale, q.rsum))) return st;
  return run_gemm_a8w8(s, EPI_STD, q.xq, q.a_scale, q.rsum, w_packed, sz_packed, nullptr, nullptr, bias, residual, y, nullptr, nullptr,
                       M, N, K, act, dtype);
}

int dihip_a8w8_norm_gemm(void* stream, const float* h, const void* gamma, float eps, const void* w_packed, const void* sz_packed,
                         const void* bias, void* y, int M, int N, int K, int act, void* ws, size_t ws_bytes, int dtype) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  A8Slices q;
  int st = a8_slices(ws, ws_bytes, M, K, &q);
  if (st) return st;
  if ((st = run_norm_act_quant(s, h, gamma, eps, M, K, dtype, q.xq, q.a_scale, q.rsum, q.tmp, q.tmp_bytes))) return st;
  return run_gemm_a8w8(s, EPI_STD, q.xq, q.a_scale, q.rsum, w_packed, sz_packed, nullptr, nullptr, bias, nullptr, y, nullptr, nullptr,
                       M, N, K, act, dtype);
}

int dihip_a8w8_norm_swiglu(void* stream, const float* h, const void* gamma, float eps, const void* wg_packed, const void* szg_packed,
                           const void* wu_packed, const void* szu_packed, void* y, int M, int N, int K, void* ws, size_t ws_bytes,
                           int dtype) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  A8Slices q;
  int st = a8_slices(ws, ws_bytes, M, K, &q);
  if (st) return st;
  if ((st = run_norm_act_quant(s, h, gamma, eps, M, K, dtype, q.xq, q.a_scale, q.rsum, q.tmp, q.tmp_bytes))) return st;
  return run_gemm_a8w8(s, EPI_SWIGLU, q.xq, q.a_scale, q.rsum, wg_packed, szg_packed, wu_packed, szu_packed, nullptr, nullptr, y,
                       nullptr, nullptr, M, N, K, DIHIP_ACT_NONE, dtype);
}

int dihip_a8w8_gemm_addto(void* stream, const void* x, const void* w_packed, const void* sz_packed, const float* h_res, float* h_out,
                          int M, int N, int K, void* ws, size_t ws_bytes, int dtype) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  A8Slices q;
  int st = a8_slices(ws, ws_bytes, M, K, &q);
  if (st) return st;
  if ((st = run_act_quant(s, x, K, M, K, dtype, q.xq, q.a_scale, q.rsum))) return st;
  return run_gemm_a8w8(s, EPI_ADDTO, q.xq, q.a_scale, q.rsum, w_packed, sz_packed, nullptr, nullptr, nullptr, nullptr, nullptr, h_res,
                       h_out, M, N, K, DIHIP_ACT_NONE, dtype);
}

}  // extern "C"
