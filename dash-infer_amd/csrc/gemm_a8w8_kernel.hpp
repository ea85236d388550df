// gemm_a8w8_kernel.hpp -- int8-activation x int8-weight GEMM for the CONTEXT phase on gfx950 (op type "GemmA8W8").
//
// Replaces GemmA8W8GPU's context-phase path (csrc/core/operator/general/gemm_lowp/gemm_a8w8_gpu.cpp:119-210): the reference
// quantises the activation rows per row (per_channel_symm_dynamic_quantization, gemm_a8w8_perc_kernel.cu:28-133, with a
// red_max / red_count spin protocol across blocks), un-reorders its N32K16 weight into a workspace on every forward (:168-179),
// runs an int8 tensor-core GEMM and dequantises in a last pass (A_perc_symm_B_perc_asymm_dequantization, :400-469).  Here:
//
//   * the quantiser (gemm_a8w8.hip) is ONE launch, one workgroup per row, the row held in registers: int8 rows padded with
//     zeros to the 64-wide k-tile, a_scale f32 [M], rsum i32 [M];
//   * B is the packed weight of the weight-only kernels, unchanged (gemm_lowp.hip: pack_w8_kernel): per 16-column tile and
//     64-k tile one 16-byte chunk per lane (kb, n) = the 16 k-values  ks * 32 + kb * 8 + j  (ks < 2, j < 8) of column n as
//     u8 = q + 128.  One xor with 0x80808080 per dword restores the signed bytes and the chunk IS the B operand of
//     v_mfma_i32_16x16x64_i8.  Integer sums do not depend on the order of k: the A operand only has to hold, in byte i of lane
//     group kb, the same k as byte i of the B chunk -- lane (kb, row) takes the two 8-byte pieces  kb * 8  and  32 + kb * 8  of
//     the row's k-tile.  One copy of the weights serves both phases.  Padding bytes of the packed image are u8 0 = -128 after
//     the flip: the padded k of A are zero (the quantiser writes them), padded columns are masked on store;
//   * workgroup tile 128 rows x 256 columns, 8 waves side by side in N (each 8 row tiles x 2 column tiles: 16 i32x4
//     accumulators), K walked in steps of A8_KB k-tiles: A goes global -> registers -> LDS once per workgroup and step, stored
//     as MFMA A fragments (one fragment = one contiguous 1 KiB), double-buffered, ONE barrier per step (A8_KB x 16 MFMAs per
//     wave between barriers); B never touches LDS;
//   * no expansion and no per-group fix-up: the products are exact in i32 (K <= 131072), and the scale / zero-point are applied
//     ONCE per output element, each line one IEEE f32 operation in the reference's order (the library is built with
//     -ffp-contract=off):
//         f = float(acc) - float(zero[n]) * float(rsum[m]);  f = f * (a_scale[m] * float(scale[n]));  f = f + bias[n];  y = FT(f)
//     then, if an activation is set, FT(act(float(y))); an FT residual is added to the rounded value as in the weight-only kernels;
//   * epilogues: STD, SwiGLU over a gate / up pair sharing one quantised A -- FT(FT(SiLU(FT(gate))) * FT(up)), the reference's
//     GemmA8W8(SILU), GemmA8W8, Binary MUL --, ADDTO: h_out = h_res + f on the f32 hidden stream.
//
// Rows >= M are clamped on load and masked on store; k-tiles past the last one of a step multiply a zero A fragment.
#pragma once
#include "gemm_lowp_kernel.hpp"

namespace dihip {

typedef int i32x4_t __attribute__((ext_vector_type(4)));

constexpr int A8_WAVES = 8;
constexpr int A8_THREADS = A8_WAVES * 64;
constexpr int A8_BM = 128;            // rows per workgroup
constexpr int A8_RT = A8_BM / 16;     // row tiles (= waves: wave w stages row tile w)
constexpr int A8_CW = 2;              // column tiles per wave
constexpr int A8_KB = 4;              // k-tiles (of 64) per step = per barrier
constexpr size_t A8_ABYTES = (size_t)A8_KB * A8_RT * 1024;  // one A buffer
constexpr size_t A8_LDS_BYTES = 2 * A8_ABYTES;
static_assert(A8_RT == A8_WAVES, "one staged row tile per wave");
static_assert(A8_LDS_BYTES <= 64 * 1024, "no dynamic-LDS grant needed");

struct A8Args {
  const u32x4_t* w0;
  const u32x4_t* w1;     // EPI_SWIGLU: "up" weight
  const uint32_t* sz0;   // [NTILES][1][16] (scale | zero << 16), per-channel
  const uint32_t* sz1;
  const int8_t* xq;      // [M, ldq] int8 rows, zero beyond K
  int ldq;               // KT * 64
  const float* a_scale;  // [M]
  const int* rsum;       // [M]
  const void* bias;      // FT [N] or null (EPI_STD)
  const void* residual;  // FT [M, N] or null (EPI_STD)
  void* y;               // FT [M, N]
  const float* h_res;    // EPI_ADDTO: f32 [M, N] or null
  float* h_out;          // EPI_ADDTO: f32 [M, N]
  int act;
  int M, N;
  int KT;                // 64-wide k-tiles
  int NTILES;            // 16-column tiles
};

// the scale / zero-point fix-up of one output element: every line ONE f32 operation (no contraction: -ffp-contract=off)
__device__ __forceinline__ float a8w8_dequant(int acc, float zero, float rsum_f, float a_scale, float scale) {
  const float zr = zero * rsum_f;
  const float f = (float)acc - zr;
  const float s = a_scale * scale;
  return f * s;
}

template <int FT, int EPI>
__global__ __launch_bounds__(A8_THREADS, 2) void gemm_a8w8_kernel(const A8Args a) {
  constexpr bool DUAL = EPI == EPI_SWIGLU;
  constexpr int HCW = A8_CW / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ni = lane & 15, kb = lane >> 4;
  // consecutive workgroups share a column block (its weights stay hot in the L2s) and walk the rows
  const int mblocks = (a.M + A8_BM - 1) / A8_BM;
  const int cb = blockIdx.x / mblocks, mb = blockIdx.x - cb * mblocks;
  const int m0 = mb * A8_BM;

  // ---- this wave's column tiles: STD / ADDTO: A8_CW consecutive tiles;  SwiGLU: the SAME tile of gate and of up
  int tile[A8_CW];
  bool tile_ok[A8_CW];
  const u32x4_t* wp[A8_CW];
#pragma unroll
  for (int c = 0; c < A8_CW; ++c) {
    const int t = DUAL ? (cb * A8_WAVES + wave) * HCW + (c % HCW) : (cb * A8_WAVES + wave) * A8_CW + c;
    tile_ok[c] = t < a.NTILES;
    tile[c] = min(t, a.NTILES - 1);
    wp[c] = ((DUAL && c >= HCW) ? a.w1 : a.w0) + (size_t)tile[c] * a.KT * 64 + lane;
  }

  // ---- A staging: wave w stages row tile w: lane (kb, r) <- bytes kb * 8 .. + 8 and 32 + kb * 8 .. + 8 of each k-tile of its row
  const int arow = min(m0 + wave * 16 + ni, a.M - 1);  // rows past M re-read the last row (masked on store)
  const int8_t* xrow = a.xq + (size_t)arow * a.ldq + kb * 8;
  u32x4_t areg[A8_KB];
  u32x4_t wreg[A8_CW][A8_KB];
  auto load_a = [&](int step) {
#pragma unroll
    for (int t = 0; t < A8_KB; ++t) {
      const int kt = step * A8_KB + t;
      if (kt < a.KT) {  // (uniform)
        const u32x2_t lo = *reinterpret_cast<const u32x2_t*>(xrow + (size_t)kt * 64);
        const u32x2_t hi = *reinterpret_cast<const u32x2_t*>(xrow + (size_t)kt * 64 + 32);
        areg[t] = u32x4_t{lo[0], lo[1], hi[0], hi[1]};
      } else {
        areg[t] = u32x4_t{0u, 0u, 0u, 0u};  // past K: a zero A fragment, whatever B holds
      }
    }
  };
  auto load_b = [&](int step) {
#pragma unroll
    for (int c = 0; c < A8_CW; ++c)
#pragma unroll
      for (int t = 0; t < A8_KB; ++t) {
        const int kt = min(step * A8_KB + t, a.KT - 1);
        wreg[c][t] = __builtin_nontemporal_load(wp[c] + (size_t)kt * 64);
      }
  };
  auto stage_a = [&](int buf) {
    unsigned char* dst = smem + buf * A8_ABYTES + ((size_t)wave * 64 + lane) * 16;
#pragma unroll
    for (int t = 0; t < A8_KB; ++t) *reinterpret_cast<u32x4_t*>(dst + (size_t)t * A8_RT * 1024) = areg[t];
  };

  i32x4_t acc[A8_RT][A8_CW];
#pragma unroll
  for (int rt = 0; rt < A8_RT; ++rt)
#pragma unroll
    for (int c = 0; c < A8_CW; ++c) acc[rt][c] = i32x4_t{0, 0, 0, 0};

  const int steps = (a.KT + A8_KB - 1) / A8_KB;
  load_a(0);
  load_b(0);
  stage_a(0);
  __syncthreads();

  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    u32x4_t wcur[A8_CW][A8_KB];
#pragma unroll
    for (int c = 0; c < A8_CW; ++c)
#pragma unroll
      for (int t = 0; t < A8_KB; ++t) wcur[c][t] = wreg[c][t];
    const bool more = s + 1 < steps;
    if (more) {  // (uniform) the loads of the next step fly while this one is multiplied
      load_a(s + 1);
      load_b(s + 1);
    }
    const unsigned char* abase = smem + buf * A8_ABYTES + (size_t)lane * 16;
#pragma unroll
    for (int t = 0; t < A8_KB; ++t) {
      i32x4_t bf[A8_CW];
#pragma unroll
      for (int c = 0; c < A8_CW; ++c) {
        const u32x4_t w = wcur[c][t];  // u8 = q + 128 -> signed bytes
        bf[c] = __builtin_bit_cast(i32x4_t, u32x4_t{w[0] ^ 0x80808080u, w[1] ^ 0x80808080u, w[2] ^ 0x80808080u, w[3] ^ 0x80808080u});
      }
#pragma unroll
      for (int rt = 0; rt < A8_RT; ++rt) {
        const i32x4_t af = *reinterpret_cast<const i32x4_t*>(abase + ((size_t)t * A8_RT + rt) * 1024);
#pragma unroll
        for (int c = 0; c < A8_CW; ++c) acc[rt][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[c], acc[rt][c], 0, 0, 0);
      }
    }
    // the next A tile into the other buffer (its last readers passed the previous barrier)
    if (more) stage_a(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: lane (kb, ni) holds rows rt * 16 + kb * 4 + r of column tile c, column ni --------------------
  float sc[A8_CW], zp[A8_CW];
#pragma unroll
  for (int c = 0; c < A8_CW; ++c) {
    const uint32_t szv = ((DUAL && c >= HCW) ? a.sz1 : a.sz0)[(size_t)tile[c] * 16 + ni];
    sc[c] = ft_bits_to_f32<FT>(szv & 0xFFFFu);
    zp[c] = ft_bits_to_f32<FT>(szv >> 16);
  }
#pragma unroll
  for (int rt = 0; rt < A8_RT; ++rt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + rt * 16 + kb * 4 + r;
      if (m >= a.M) continue;
      const float as = a.a_scale[m], rs = (float)a.rsum[m];
      if constexpr (DUAL) {
#pragma unroll
        for (int c = 0; c < HCW; ++c) {
          const int n = tile[c] * 16 + ni;
          if (tile_ok[c] && n < a.N) {
            const float g = ft_round<FT>(a8w8_dequant(acc[rt][c][r], zp[c], rs, as, sc[c]));
            const float u = ft_round<FT>(a8w8_dequant(acc[rt][HCW + c][r], zp[HCW + c], rs, as, sc[HCW + c]));
            const float sg = ft_round<FT>(g / (1.f + expf(-g)));
            store_ft<FT>(a.y, (size_t)m * a.N + n, sg * u);
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < A8_CW; ++c) {
          const int n = tile[c] * 16 + ni;
          if (!tile_ok[c] || n >= a.N) continue;
          float v = a8w8_dequant(acc[rt][c][r], zp[c], rs, as, sc[c]);
          if constexpr (EPI == EPI_STD) {
            if (a.bias) v = v + load_ft<FT>(a.bias, n);
            if (a.act != DIHIP_ACT_NONE) v = apply_act(ft_round<FT>(v), a.act);
            if (a.residual) v = ft_round<FT>(v) + load_ft<FT>(a.residual, (size_t)m * a.N + n);
            store_ft<FT>(a.y, (size_t)m * a.N + n, v);
          } else {
            const float base = a.h_res ? a.h_res[(size_t)m * a.N + n] : 0.f;
            a.h_out[(size_t)m * a.N + n] = base + v;
          }
        }
      }
    }
  }
}

template <int FT, int EPI>
hipError_t launch_gemm_a8w8(const A8Args& a, int blocks, hipStream_t stream);

#define DIHIP_DEFINE_A8W8_LAUNCH(FT, EPI)                                                                          \
  template <>                                                                                                      \
  hipError_t launch_gemm_a8w8<FT, EPI>(const A8Args& a, int blocks, hipStream_t s) {                               \
    hipLaunchKernelGGL((gemm_a8w8_kernel<FT, EPI>), dim3(blocks), dim3(A8_THREADS), A8_LDS_BYTES, s, a);           \
    return hipGetLastError();                                                                                      \
  }

#define DIHIP_DEFINE_A8W8_LAUNCH_SET(FT)     \
  DIHIP_DEFINE_A8W8_LAUNCH(FT, EPI_STD)      \
  DIHIP_DEFINE_A8W8_LAUNCH(FT, EPI_SWIGLU)   \
  DIHIP_DEFINE_A8W8_LAUNCH(FT, EPI_ADDTO)

}  // namespace dihip
