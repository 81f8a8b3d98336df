// 3x3 / stride 1 / pad 1 convolution of the full-resolution decoder head, NHWC, as an
// implicit GEMM on MFMA with an LDS halo tile.  Replaces FinalPatchExpand_X4_V2's
// refine1 / refine2 (network/model_parts.py:447-448, :468-471) together with the ops
// around them:
//   * depth-to-space 4x4 of the expand output (model_parts.py:464-465) is folded into the
//     input addressing (IN_D2S) -- the d2s tensor and the NHWC->NCHW permute never exist;
//   * GELU of the conv input (model_parts.py:460, :469) comes from the producer: its epilogue
//     stores GELU(Y) beside the pre-activation Y (DUAL), and the conv loads that activation as
//     it is (ops.refine_conv_act, the model's path).  GELU on load (IN_GELU, ops.refine_conv)
//     is kept for tests and tools: the generic kernel and the weight gradients have it;
//   * bias add in the epilogue; backward-data multiplies by GELU'(pre-activation) in the
//     epilogue and scatters through the same d2s map (OUT_D2S / OUT_GGRAD).
// fwd and dgrad share one kernel (dgrad = conv with spatially flipped, ci<->co swapped
// weights): conv3x3_kernel for any width and dtype, conv3x3_v3_kernel (persistent, LDS-DMA)
// for 16-bit C = 96 and 128 without GELU on load; persistent_width() picks.  wgrad reads both
// operands k-strided from natural [pixel][channel] LDS images with ds_read_b64_tr_b16 (bf16)
// and writes deterministic per-block partials.
#pragma once
#include <cstdlib>
#include <utility>

#include "common.h"
#include "mfma_frag.h"
#include "reduce.h"

// msu_conv_mode (defined in conv3x3.hip, one copy for both translation units).
// bit 0 (default on; A/B switch MSU_CONV_DYN): conv3x3_v3_kernel takes tiles from the
// per-stream queue slot instead of the static blockIdx.x + k * gridDim.x schedule
extern int g_conv_dyn;
// bit 1 (default off; the A/B handle of tools and tests, no environment switch): widths other
// than 96 take the generic kernels
extern int g_conv_generic_wide;

// MSU_EXP: ablation bits for timing experiments only (tools/build_exp.sh); 0 in every real build
#ifndef MSU_EXP
#define MSU_EXP 0
#endif

namespace {

constexpr int TW = 16;  // output tile width (pixels) = one MFMA M tile

struct ConvGeom {
  int B, H, W;
  int Cin, CinP;   // GEMM input channels, padded to a multiple of 32
  int Cout;        // GEMM output channels (multiple of 16)
  int PS;          // LDS pixel stride (elements) of the input image
  int PSW;         // LDS row stride of the weight tile (fwd/dgrad)
  int PSD;         // LDS pixel stride of the dY tile (wgrad)
};

// element offset of channel 0 of pixel (b, y, x) of the logical [B,H,W,C] image
template <bool D2S>
MSU_DEV long pix_off(int b, int y, int x, int H, int W, int C) {
  if constexpr (D2S) {
    const int h4 = H >> 2, w4 = W >> 2;
    return (((long)b * h4 + (y >> 2)) * w4 + (x >> 2)) * (16L * C) + (long)(((y & 3) * 4 + (x & 3)) * C);
  } else {
    return (((long)b * H + y) * W + x) * (long)C;
  }
}

// 32-bit variant (tensors below 2^31 elements; checked on the host)
template <bool D2S>
MSU_DEV int pix_off32(int b, int y, int x, int H, int W, int C) {
  if constexpr (D2S) {
    const int h4 = H >> 2, w4 = W >> 2;
    return ((b * h4 + (y >> 2)) * w4 + (x >> 2)) * (16 * C) + ((y & 3) * 4 + (x & 3)) * C;
  } else {
    return ((b * H + y) * W + x) * C;
  }
}

// Stage rows [y_first, y_first + nrows) x cols [x0 - 1, x0 + TW + 1) of the transformed
// input image (GELU optional) into LDS sX[(row * (TW+2) + col) * PS + c]; zero outside.
template <typename T, bool D2S, bool GELU>
MSU_DEV void stage_halo(const T* X, T* sX, int b, int y_first, int nrows, int x0, const ConvGeom& g,
                        int tid, int nthreads) {
  const int cpp = g.CinP / 8;  // 8-element chunks per pixel
  const int total = nrows * (TW + 2) * cpp;
  for (int i = tid; i < total; i += nthreads) {
    const int pix = i / cpp, ch = i - pix * cpp;
    const int row = pix / (TW + 2), col = pix - row * (TW + 2);
    const int y = y_first + row, x = x0 - 1 + col;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (y >= 0 && y < g.H && x >= 0 && x < g.W && ch * 8 < g.Cin) {
      const T* p = X + pix_off<D2S>(b, y, x, g.H, g.W, g.Cin) + ch * 8;
      float a[4], c[4];
      Vec4<T>::load(p, a);
      Vec4<T>::load(p + 4, c);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = c[e]; }
      if constexpr (GELU) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = gelu_f(v[e]);
      }
    }
    T* d = sX + pix * g.PS + ch * 8;
    float lo[4] = {v[0], v[1], v[2], v[3]}, hi[4] = {v[4], v[5], v[6], v[7]};
    Vec4<T>::store(d, lo);
    Vec4<T>::store(d + 4, hi);
  }
}

// acc += A(16 x 32) B(32 x 16) with both operands k-contiguous in LDS.
template <typename T> struct KC;
template <typename T> struct KC16 {
  static MSU_DEV void mma(f32x4& acc, const T* A, int lda, const T* B, int ldb, int lane) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(A + (lane & 15) * lda + 8 * (lane >> 4));
    const bf16x8 b = *reinterpret_cast<const bf16x8*>(B + (lane & 15) * ldb + 8 * (lane >> 4));
    acc = Fmt16<T>::mma16(a, b, acc);
  }
};
template <> struct KC<bf16_t> : KC16<bf16_t> {};
template <> struct KC<f16_t> : KC16<f16_t> {};
template <> struct KC<float> {
  static MSU_DEV void mma(f32x4& acc, const float* A, int lda, const float* B, int ldb, int lane) {
    const float* pa = A + (lane & 15) * lda + (lane >> 4);
    const float* pb = B + (lane & 15) * ldb + (lane >> 4);
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[4 * s], pb[4 * s], acc, 0, 0, 0);
  }
};

// ------------------------------------------------------------------ fwd / dgrad kernel
// Y[pixel][co] = sum_{tap, ci} Xt[pixel + off(tap)][ci] * Wt[tap][co][ci] (+ bias[co])
//               (* GELU'(S[pixel][co]) when OUT_GGRAD), Xt = GELU?(map(X));
// DUAL: Y2 = GELU(Y) as well (the following conv then loads it without converting).
// Block = NWAVES waves = TH x 16 output pixels x all Cout; wave w owns MT image rows.
template <typename T, int NT, int TH, int MT, bool DB, bool IN_D2S, bool IN_GELU, bool OUT_D2S,
          bool OUT_GGRAD, bool BIAS, bool DUAL>
__global__ void __launch_bounds__(64 * (TH / MT)) conv3x3_kernel(const T* __restrict__ X,
                                                                 const T* __restrict__ Wt,
                                                                 const float* __restrict__ bias,
                                                                 const T* __restrict__ S,
                                                                 T* __restrict__ Y, T* __restrict__ Y2,
                                                                 ConvGeom g) {
  constexpr int NWAVES = TH / MT;
  constexpr int NTHR = 64 * NWAVES;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* sX = reinterpret_cast<T*>(smem_raw);
  T* sW0 = sX + (TH + 2) * (TW + 2) * g.PS;
  T* sW1 = sW0 + g.Cout * g.PSW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (g.W + TW - 1) / TW, tiles_y = (g.H + TH - 1) / TH;
  const long ntiles = (long)g.B * tiles_x * tiles_y;
  const long tile = xcd_remap(blockIdx.x, gridDim.x);
  if (tile >= ntiles) return;
  const int b = (int)(tile / ((long)tiles_x * tiles_y));
  const int trem = (int)(tile - (long)b * tiles_x * tiles_y);
  const int y0 = (trem / tiles_x) * TH, x0 = (trem % tiles_x) * TW;

  stage_halo<T, IN_D2S, IN_GELU>(X, sX, b, y0 - 1, TH + 2, x0, g, tid, NTHR);
  // weight tile of tap t: Wt[t] is [Cout][CinP] contiguous -> sW[co * PSW + ci]
  const int wchunks = g.Cout * (g.CinP / 8);
  auto load_w = [&](int t, T* dst) {
    const T* src = Wt + (long)t * g.Cout * g.CinP;
    for (int i = tid; i < wchunks; i += NTHR) {
      const int co = i / (g.CinP / 8), ch = i - co * (g.CinP / 8);
      *reinterpret_cast<uint4*>(dst + co * g.PSW + ch * 8) =
          *reinterpret_cast<const uint4*>(src + (long)co * g.CinP + ch * 8);
    }
  };
  static_assert(sizeof(T) == 2 || !DB, "double-buffered weights only for bf16");
  if constexpr (sizeof(T) == 2) {
    load_w(0, sW0);
  } else {
    // f32: 8-element chunks are 32 bytes
    const float* src = reinterpret_cast<const float*>(Wt);
    for (int i = tid; i < g.Cout * g.CinP; i += NTHR) {
      const int co = i / g.CinP, ci = i - co * g.CinP;
      reinterpret_cast<float*>(sW0)[co * g.PSW + ci] = src[i];
    }
  }
  __syncthreads();

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nks = g.CinP / 32;
  for (int tap = 0; tap < 9; ++tap) {
    const int dy = tap / 3, dx = tap - (tap / 3) * 3;
    T* sW = (DB && (tap & 1)) ? sW1 : sW0;
    if constexpr (DB) {
      if (tap + 1 < 9) load_w(tap + 1, (tap & 1) ? sW0 : sW1);
    }
    for (int ks = 0; ks < nks; ++ks) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int hrow = wave * MT + m + dy;  // halo row
        const T* A = sX + (hrow * (TW + 2) + dx) * g.PS + ks * 32;
#pragma unroll
        for (int n = 0; n < NT; ++n)
          KC<T>::mma(acc[m][n], A, g.PS, sW + n * 16 * g.PSW + ks * 32, g.PSW, lane);
      }
    }
    __syncthreads();
    if constexpr (!DB) {
      if (tap + 1 < 9) {
        if constexpr (sizeof(T) == 2) {
          load_w(tap + 1, sW0);
        } else {
          const float* src = reinterpret_cast<const float*>(Wt) + (long)(tap + 1) * g.Cout * g.CinP;
          for (int i = tid; i < g.Cout * g.CinP; i += NTHR) {
            const int co = i / g.CinP, ci = i - co * g.CinP;
            reinterpret_cast<float*>(sW0)[co * g.PSW + ci] = src[i];
          }
        }
        __syncthreads();
      }
    }
  }

  // epilogue: lane holds pixel x0 + (lane>>4)*4 + r of row y0 + wave*MT + m, channel n*16 + (lane&15)
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int y = y0 + wave * MT + m;
    if (y >= g.H) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int x = x0 + (lane >> 4) * 4 + r;
      if (x >= g.W) continue;
      const long base = pix_off<OUT_D2S>(b, y, x, g.H, g.W, g.Cout);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int co = n * 16 + (lane & 15);
        float v = acc[m][n][r];
        if constexpr (BIAS) v += bias[co];
        if constexpr (OUT_GGRAD) v *= gelu_grad_f(to_f32(S[base + co]));
        Y[base + co] = from_f32<T>(v);
        // DUAL: also GELU of the stored (rounded) value -- the next conv's input
        if constexpr (DUAL) Y2[base + co] = from_f32<T>(gelu_f(to_f32(from_f32<T>(v))));
      }
    }
  }
}

// ------------------------------------------------------------------ 16-bit helpers
// Shared by the persistent kernels below (conv3x3_v3_kernel, conv3x3_wgrad_v2_kernel): eight
// 16-bit values of a 16-B chunk as floats, GELU of a chunk in registers (the DUAL epilogue, the
// weight gradient's in-place conversion), and a compile-time loop over integral constants.
template <typename T> MSU_DEV void unpack8(const u32x4& q, float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = Fmt16<T>::lo(q[i]);
    v[2 * i + 1] = Fmt16<T>::hi(q[i]);
  }
}
template <typename T> MSU_DEV u32x4 gelu8(const u32x4& q) {
  float v[8];
  unpack8<T>(q, v);
  return u32x4{pack2<T>(gelu_fast(v[0]), gelu_fast(v[1])), pack2<T>(gelu_fast(v[2]), gelu_fast(v[3])),
               pack2<T>(gelu_fast(v[4]), gelu_fast(v[5])), pack2<T>(gelu_fast(v[6]), gelu_fast(v[7]))};
}

template <int I> using IC = std::integral_constant<int, I>;
template <typename F, int... Is>
MSU_DEV void static_for(F&& f, std::integer_sequence<int, Is...>) {
  (f(IC<Is>{}), ...);
}

// ------------------------------------------------------------------ 16-bit fwd / dgrad, v3 (C = 96, 128)
// Persistent implicit GEMM on v_mfma_f32_{32x32x16,16x16x32}_{bf16,f16} (raw 16-bit storage;
// T = format): one workgroup of 8 waves per CU loops over output tiles, D[co][pixel] =
// W_tap[co][ci] * X[ci][pixel] with the weight fragment as the A operand, so each lane ends
// with consecutive output channels of one pixel.  The plain plan (8 waves x one output row,
// padded LDS images, weights staged through registers) spends as many LDS cycles as MFMA
// cycles: per tap and wave 24 ds_read_b128 for 18 MFMAs, plus 24 KB of weight ds_writes per
// tap.  v3 halves both per output pixel:
//   * a tile is 16 rows x 32 pixels x 96 channels; wave w owns rows 2w, 2w + 1, so each weight
//     fragment feeds two MFMAs (reads per MFMA 5/6 instead of 4/3);
//   * the halo [18][34][96] and the weight image of a tap [96][96] are stored UNPADDED with
//     the 16-B chunk c of row / pixel p at c ^ ((p >> 2) & 3): a half-wave's fragment read
//     (32 consecutive rows, one chunk) covers all 64 banks, and the 154 KB of LDS fit;
//   * the weights of tap t + 1 arrive by LDS-DMA (global_load_lds_dwordx4, source addresses
//     permuted by the same swizzle) into the other of two weight images while tap t runs --
//     no registers and no ds_write for the weight ring, one barrier per tap;
//   * the next tile's halo is loaded into registers at tap 1 and written to LDS after tap 8.
// Epilogue: bias, DUAL = GELU(Y) as a second output, GELU'(S) for the backward-data launches
// with S prefetched at tap 7, 16-B stores after a permlane32 (16x16x32: permlane16) swap.
//
// C = 128 (Swin-B) is the same kernel at another width: every count below comes from V3W<C>.
// Its 18 x 34 halo would be 157 KB, so a tile is 8 rows x 32 pixels (one row per wave; halo
// [10][34][128] = 85 KB + two 32 KB weight images), and all of its launches run on 16x16x32
// MFMA, where a weight fragment still feeds two MFMAs (the two 16-pixel halves of the row).
constexpr int V3_HALO_TAP = 1;
// ablation bit 1024: all GELU' operands at tap 7 (the round-5 placement; spilled halo registers)
constexpr bool SP_AT7 = (MSU_EXP & 1024) != 0;

// Widths the kernel is built for (Cin == Cout == C) and everything derived from them.
// TWV_: tile width in pixels; C = 128 fits 8 rows x 32 pixels (one row per wave) or 16 rows x
// 16 pixels (two rows per wave) beside its weight images
template <int C_, int TWV_ = 32>
struct V3W {
  static_assert(C_ == 96 || C_ == 128, "widths with a register plan and a conflict-free LDS image");
  static_assert(TWV_ == 32 || (C_ == 128 && TWV_ == 16), "tile widths");
  static constexpr int C = C_;
  static constexpr int CH = C / 8;               // 16-B chunks per pixel / weight row
  static constexpr int NW = 8;                   // waves
  static constexpr int MT = C == 96 || TWV_ == 16 ? 2 : 1;  // image rows per wave
  static constexpr int TH = NW * MT, TWV = TWV_, HWD = TWV + 2;
  static constexpr int PT = TWV / 16;            // 16-pixel tiles per row (16x16x32 form)
  static constexpr int HPIX = (TH + 2) * HWD;    // halo pixels (612 / 340 / 324)
  static constexpr int NQ = C / 32;              // 32-channel groups: a lane's 16-B stores per pixel
  static constexpr int NT32 = C / 32, KS32 = C / 16;  // 32x32x16 form: co tiles, k steps
  static constexpr int NT16 = C / 16, KS16 = C / 32;  // 16x16x32 form
  static constexpr int WIMG = C * C;             // elements of one tap's weight image
  static constexpr int WINS = WIMG * 2 / 1024;   // 1-KB DMA wave-instructions per tap (18 / 32)
  static constexpr int WPER = (WINS + NW - 1) / NW;   // per wave (<= 3 / 4)
  static_assert(WINS * 1024 == WIMG * 2, "weight image in whole DMA instructions");
  // GELU' operand loads per lane (dgrad): the first 32-channel group at tap 7, the rest at tap 8
  static constexpr int SPRE = MT * PT * NQ;
  static constexpr int SP7 = SP_AT7 ? SPRE : SPRE / NQ;
  // halo + two weight images + bias + queue entry
  static constexpr size_t LDS = sizeof(bf16_t) * ((size_t)HPIX * C + 2 * WIMG) + C * sizeof(float) + 16;
  static_assert(LDS <= 160 * 1024, "LDS");
  // the 32x32x16 form's k-step addressing assumes the 2-bit swizzle of the 192-B rows
  template <bool M16> static constexpr bool form_ok = M16 || (C == 96 && TWV == 32);
};

// ---- LDS images.  Halo pixels and weight rows are unpadded [.][C]; the 16-B chunk c of row /
// pixel p sits at chunk slot c ^ v3_swz(p).  The fragment reads, the halo stores and the DMA's
// source permutation all go through v3_slot, and the asserts below check reads and DMA.
//   C = 96 (192-B rows, two rows to three bank spans): (p >> 2) & 3 for the 32x32x16 form
//   (a half-wave reads 32 consecutive rows, one chunk) and (p >> 1) & 3 for 16x16x32;
//   C = 128: a row is one whole 256-B bank span, every row starts on bank 0, and a 2-bit
//   swizzle leaves 16 rows on 4 columns.  (p & 7) << 1 moves the chunk's bits 1-3: a
//   ds_read_b128 lane group holds 8 consecutive pixels with an even chunk and the 8 that follow
//   with the next odd one, so each parity's 8 pixels take the 8 columns of that parity.
#define V3_MAP __host__ __device__ __forceinline__ constexpr
template <int C, bool M16> V3_MAP int v3_swz(int p) {
  return C == 128 ? (p & 7) << 1 : M16 ? (p >> 1) & 3 : (p >> 2) & 3;
}
// element offset of chunk c of row / pixel p
template <int C, bool M16> V3_MAP int v3_slot(int p, int c) { return p * C + ((c ^ v3_swz<C, M16>(p)) << 3); }
// 16x16x32 form: k step ks of the fragment whose k step 0 is at `off` = v3_slot(p, lane >> 4).
// The 2-bit swizzle stays inside a k step's four chunks (an immediate offset); the C = 128 one
// does not, but rows are 128 elements, so the chunk's k-step bits flip in place.
template <int C> V3_MAP int v3_kstep(int off, int ks) { return C == 128 ? off ^ (32 * ks) : off + 32 * ks; }
// the weight DMA's 16-B piece q lands at byte 16 q of the image: row q / CH takes this chunk
template <int C, bool M16> V3_MAP int v3_dma_chunk(int q) { return (q % (C / 8)) ^ v3_swz<C, M16>(q / (C / 8)); }

// ds_read_b128 resolves bank conflicts within four groups of 16 lanes: lanes {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same plus 32.  Lane i (0 .. 15) of group g (0 .. 3):
constexpr int v3_b128_lane(int g, int i) {
  const int l = (g & 1) == 0 ? (i < 4 ? i : i < 8 ? i + 8 : i + 12) : (i < 8 ? i + 4 : i < 12 ? i + 8 : i + 16);
  return l + 32 * (g >> 1);
}
// every 16x16x32 fragment read (16 consecutive rows / pixels from ANY first one -- the halo
// reads start at (row + dy) * 34 + dx + 16 pt --, chunk 4 ks + (lane >> 4)) puts each group's
// 16 lanes on 16 distinct 16-B bank columns
template <int C>
constexpr bool v3_reads_conflict_free() {
  for (int p0 = 0; p0 < 64; ++p0)
    for (int ks = 0; ks < V3W<C>::KS16; ++ks)
      for (int g = 0; g < 4; ++g) {
        unsigned cols = 0;
        for (int i = 0; i < 16; ++i) {
          const int lane = v3_b128_lane(g, i);
          const int off = v3_kstep<C>(v3_slot<C, true>(p0 + (lane & 15), lane >> 4), ks);
          cols |= 1u << ((off >> 3) & 15);
        }
        if (cols != 0xffffu) return false;
      }
  return true;
}
// the DMA writes the image the reads expect, and every k step reads its own four chunks
template <int C, bool M16>
constexpr bool v3_dma_writes_image() {
  for (int q = 0; q < V3W<C>::WIMG / 8; ++q)
    if (v3_slot<C, M16>(q / V3W<C>::CH, v3_dma_chunk<C, M16>(q)) != 8 * q) return false;
  for (int p = 0; p < 64; ++p)
    for (int ks = 0; ks < V3W<C>::KS16; ++ks)
      for (int g4 = 0; g4 < 4; ++g4)
        if (v3_kstep<C>(v3_slot<C, true>(p, g4), ks) != v3_slot<C, true>(p, 4 * ks + g4)) return false;
  return true;
}
static_assert(v3_reads_conflict_free<96>() && v3_reads_conflict_free<128>(), "halo / weight image: bank conflicts");
static_assert(v3_dma_writes_image<96, true>() && v3_dma_writes_image<96, false>() && v3_dma_writes_image<128, true>(),
              "weight image: DMA and reads disagree");

// SPREAD: the next tile's halo loads are issued in seven parts at taps 1..7 (each part issued
// after that tap's weight DMA, so it only has to land two taps later) instead of all at tap 1,
// where the wait for tap 3's weights also waited for the whole 117 KB halo.
MSU_DEV constexpr int halo_part_lo(int t, int nhc) { return (t - 1) * nhc / 7; }  // t = 1..7

// Tile queue (tq, common.h): a workgroup takes its first tile statically (blockIdx.x) and claims
// every further one from counter 0, one tile ahead (the next tile's halo and weight prefetch
// need its index from tap 1 on).  Results do not depend on which workgroup computes a tile.
template <typename T, bool IN_D2S, bool OUT_D2S, bool OUT_GGRAD, bool BIAS, bool DUAL, bool SPREAD, bool M16,
          int CW = 96, int TWW = 32>
__global__ void __launch_bounds__(512) conv3x3_v3_kernel(const bf16_t* __restrict__ X,
                                                         const bf16_t* __restrict__ Wt,
                                                         const float* __restrict__ bias,
                                                         const bf16_t* __restrict__ S,
                                                         bf16_t* __restrict__ Y, bf16_t* __restrict__ Y2,
                                                         ConvGeom g, int ntiles, int* __restrict__ tq) {
  using G = V3W<CW, TWW>;
  static_assert(G::template form_ok<M16>, "the 32x32x16 form is built for C = 96 only");
  constexpr int C = G::C, CH = G::CH, NW = G::NW, MT = G::MT, TH = G::TH, TWV = G::TWV, HWD = G::HWD;
  constexpr int HPIX = G::HPIX;
  (void)HPIX;
  constexpr int PT = G::PT, NQ = G::NQ, NT32 = G::NT32, KS32 = G::KS32, NT16 = G::NT16, KS16 = G::KS16;
  constexpr int NTHR = 64 * NW;
  constexpr int PSTEP = NTHR / CH;                // halo pixels per staging round (one channel
                                                  // chunk per thread: thread t stages chunk t % CH)
  constexpr int NHC = (HPIX + PSTEP - 1) / PSTEP;  // staging rounds
  constexpr int WIMG = G::WIMG;                 // elements of one tap's weight image
  constexpr int WINS = G::WINS;                 // DMA wave-instructions per tap
  constexpr int WPER = G::WPER;                 // per wave

  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16_t* sX = reinterpret_cast<bf16_t*>(smem_raw);
  bf16_t* sW = sX + HPIX * C;  // [2][C][C]
  float* sB = reinterpret_cast<float*>(sW + 2 * WIMG);  // [C] bias (BIAS)
  int* sQ = reinterpret_cast<int*>(sB + C);              // the claimed next tile (tq)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_x = (g.W + TWV - 1) / TWV, tiles_y = (g.H + TH - 1) / TH;
  // output stores of a whole tile, per wave (16-B stores; DUAL: two per output chunk)
  constexpr int EST = MT * PT * NQ * (DUAL ? 2 : 1);
  static_assert(WPER + EST < 64, "tap 0's counted wait fits vmcnt");
  const int per_img = tiles_x * tiles_y;

  auto coords = [&](int tile, int& b, int& y0, int& x0) {
    b = tile / per_img;
    const int r = tile - b * per_img;
    y0 = (r / tiles_x) * TH;
    x0 = (r - (r / tiles_x) * tiles_x) * TWV;
  };
  u32x4 hr[NHC];
  // Halo staging: thread t < CH * PSTEP owns channel chunk t % CH of pixels t / CH + PSTEP * c
  // (c = 0 .. NHC-1); the pixel's (row, col) advance incrementally, so a chunk costs a few adds
  // and one address multiply instead of the divisions of a flat chunk index
  // rounds [c0, c1) of this thread's share of tile `tile`'s halo -> registers
  auto load_halo = [&](int tile, auto C0, auto C1) {
    constexpr int c0 = decltype(C0)::value, c1 = decltype(C1)::value;
    int b, y0, x0;
    coords(tile, b, y0, x0);
    const int t = opaque(tid);  // recomputed per call: nothing pinned across the tile loop
    const bool hact = t < PSTEP * CH;
    int p = t / CH + PSTEP * c0;
    int row = p / HWD, col = p - (p / HWD) * HWD;
    const bf16_t* xc = X + (t % CH) * 8;
#pragma unroll
    for (int c = c0; c < c1; ++c) {
      const int y = y0 - 1 + row, x = x0 - 1 + col;
      const bool ok = !(MSU_EXP & 256) && hact && p < HPIX && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W;
      // out-of-image chunks read the zero region: no select on the loaded value, so the load
      // stays in flight until the halo is stored (address select, no branch)
      const bf16_t* src = ok ? xc + pix_off32<IN_D2S>(b, y, x, g.H, g.W, C)
                             : reinterpret_cast<const bf16_t*>(zero_src(tid));
      hr[c] = *reinterpret_cast<const u32x4*>(src);
      p += PSTEP;
      col += PSTEP % HWD;
      row += PSTEP / HWD;
      if (col >= HWD) {
        col -= HWD;
        ++row;
      }
    }
  };
  auto store_halo = [&]() {
    const int t = opaque(tid);
    const bool hact = t < PSTEP * CH;
    const int hch = t % CH;
    int p = t / CH;
#pragma unroll
    for (int c = 0; c < NHC; ++c) {
      if (hact && p < HPIX) *reinterpret_cast<u32x4*>(sX + v3_slot<C, M16>(p, hch)) = hr[c];
      p += PSTEP;
    }
  };
  // this wave's share of the DMA of tap `tap`'s weight image into buffer `buf`
  auto dma_w = [&](int tap, int buf) {
    const bf16_t* src = Wt + (long)tap * WIMG;
    bf16_t* dst = sW + buf * WIMG;
    // piece r of this wave is slot q = 64 (wave + NW r) + lane: row q / CH, chunk q % CH,
    // advanced incrementally from r = 0 (one division per call)
    const int q0 = 64 * wave + opaque(lane);
    int row = q0 / CH, pos = q0 - (q0 / CH) * CH;
#pragma unroll
    for (int r = 0; r < WPER; ++r) {
      const int k = wave + NW * r;
      if (WINS % NW == 0 || k < WINS) glds16((MSU_EXP & 512) ? src + lane * 8 : src + v3_slot<C, M16>(row, pos), dst + 512 * k);
      pos += (64 * NW) % CH;
      row += (64 * NW) / CH;
      if (pos >= CH) {
        pos -= CH;
        ++row;
      }
    }
  };
  // DMA wave-instructions this wave issues per tap (wave-uniform)
  const int my_wdma = (WINS - wave + NW - 1) / NW;

  // tq: claims count up from 0 (tile gridDim.x + count)
  auto finish = [&]() { tq_finish(tq); };
  // the tile thread 0 left in sQ (after a barrier); untracked read: a compiler-visible ds_read
  // would wait for the weight DMA and output stores in flight here (vmcnt(0))
  auto read_q = [&]() -> int {
    uint32_t v = ds_b32_untracked<0>(lds_u32(sQ));
    lds_wait_tie<0>(v);
    return __builtin_amdgcn_readfirstlane((int)v) + (int)gridDim.x;
  };
  int tile = blockIdx.x;
  if (tile >= ntiles) {  // (the launch keeps the grid <= ntiles)
    finish();
    return;
  }
  if (tq != nullptr && tid == 0) sQ[0] = tq_claim(tq, 0);
  if constexpr (BIAS) {
    if (tid < C) sB[tid] = bias[tid];  // read by every epilogue from LDS (no global load there)
  }
  load_halo(tile, IC<0>{}, IC<NHC>{});
  store_halo();
  dma_w(0, 0);
  __syncthreads();  // the halo's ds_writes land before any wave reads (the tap barriers are raw)
  int next = tq != nullptr ? read_q() : tile + (int)gridDim.x;
  int wbuf = 0;
  // w1_early: this tile's W(1) was DMA'd by the previous tile's epilogue, ahead of its output
  // stores; st_full: those stores are all EST of them (a whole tile) and may stay in flight
  // through tap 0 (waits at taps 0 / 1 count them) instead of draining before tap 0
  bool w1_early = false, st_full = false;

  const int xl = lane & 31, h = lane >> 5;
  // lane chunk offsets (elements) of k steps with ks even / odd, for row / pixel swizzle sw:
  // chunk 2ks + h -> 4 (ks >> 1) + ((2 (ks & 1) + h) ^ sw)
  auto koff = [&](int sw, int odd) { return ((2 * odd + h) ^ sw) << 3; };
  const int wsw = v3_swz<C, false>(xl);  // weight rows 32n + xl
  const int wk0 = xl * C + koff(wsw, 0), wk1 = xl * C + koff(wsw, 1);
  // M16: lane l reads row (l & 15) of a 16-row fragment, chunk 4 ks + (l >> 4)
  const int l15 = lane & 15, g4 = lane >> 4;
  const int wk16 = v3_slot<C, true>(l15, g4);  // weight rows 16n + l15, k step 0

  for (;;) {
    int nn = 0;  // thread 0 (tq): the tile after next, claimed at tap 1
    int b, y0, x0;
    coords(tile, b, y0, x0);
    const int xo = x0 + xl;
    // accumulators: 32x32 tiles [row m][co tile n] (!M16) or 16x16 tiles [row m][pixel tile
    // pt][co tile n] (M16); the other form is a 1-element placeholder
    f32x16 acc[M16 ? 1 : MT][M16 ? 1 : NT32];
    f32x4 acc4[M16 ? MT : 1][M16 ? PT : 1][M16 ? NT16 : 1];
    if constexpr (M16) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
          for (int n = 0; n < NT16; ++n) acc4[m][pt][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT32; ++n) acc[m][n] = f32x16{0};
    }
    // dgrad GELU' operands: SPRE 16-B pieces per lane in both forms
    u32x4 sp[OUT_GGRAD ? MT : 1][OUT_GGRAD ? (M16 ? PT : NQ) : 1][OUT_GGRAD ? (M16 ? NQ : 2) : 1];

    static_for([&](auto TAP) {
      constexpr int tap = decltype(TAP)::value;
      constexpr int dy = tap / 3, dx = tap % 3;
      // W(tap) landed (this wave's DMAs; the halo loads issued after them may stay in flight),
      // then the barrier: every wave's DMA landed, every wave done with the other buffer
      // loads issued at tap - 1 after that tap's weight DMA may stay in flight: the halo
      // part(s) of the next tile and (dgrad, tap 7) the GELU' operands
      constexpr int hprev = SPREAD ? (tap >= 2 ? halo_part_lo(tap, NHC) - halo_part_lo(tap - 1, NHC) : 0)
                                   : (tap == V3_HALO_TAP + 1 ? NHC : 0);
      // (only a third of them are issued at tap 7, see load_sp / load_sp16)
      constexpr int sprev = (OUT_GGRAD && tap == 8) ? G::SP7 : 0;
      if constexpr (tap == 0) {
        // W(0) landed (DMA'd at the previous tile's tap 8); W(1) and the previous tile's output
        // stores, issued after it in that epilogue, may stay in flight
        if (!w1_early) wait_vmcnt<0>();
        else if (st_full) {
          if (my_wdma == WPER) wait_vmcnt<WPER + EST>();
          else wait_vmcnt<WPER - 1 + EST>();
        } else {
          if (my_wdma == WPER) wait_vmcnt<WPER>();
          else wait_vmcnt<WPER - 1>();
        }
      } else if constexpr (tap == 1) {
        static_assert(hprev == 0 && sprev == 0, "tap 1 waits");
        if (w1_early && st_full) wait_vmcnt<EST>();  // W(1) is older than the stores
        else wait_vmcnt<0>();
      } else if constexpr (hprev > 0) {
        if (next < ntiles) wait_vmcnt<hprev + sprev>();
        else wait_vmcnt<sprev>();
      } else {
        wait_vmcnt<sprev>();
      }
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const bf16_t* wcur = sW + wbuf * WIMG;
      if constexpr (tap == 0) {
        if (!w1_early) dma_w(1, wbuf ^ 1);
      } else if constexpr (tap == 1) {
        // claim the tile after next (thread 0); older than W(2)'s DMA, so tap 2's counted wait
        // covers it
        // (the raw count; offset by gridDim.x on read)
        if (tq != nullptr && tid == 0 && next < ntiles) nn = tq_claim(tq, 0);
        dma_w(2, wbuf ^ 1);
      } else if constexpr (tap == 2) {
        // the claim to sQ: every wave read this tile's entry before tap 0's barrier, the next
        // read follows the tile's closing barrier.  Untracked write (a visible ds_write would
        // wait for the weight DMA in flight).
        if (tq != nullptr && tid == 0 && next < ntiles) {
          asm volatile("ds_write_b32 %0, %1" ::"v"(lds_u32(sQ)), "v"(nn) : "memory");
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        dma_w(3, wbuf ^ 1);
      } else if constexpr (tap < 8) {
        dma_w(tap + 1, wbuf ^ 1);
      } else {
        if (next < ntiles) dma_w(0, wbuf ^ 1);
      }
      if constexpr (SPREAD && tap >= 1 && tap <= 7) {
        if (next < ntiles) load_halo(next, IC<halo_part_lo(tap, NHC)>{}, IC<halo_part_lo(tap + 1, NHC)>{});
      } else if constexpr (!SPREAD && tap == V3_HALO_TAP) {
        if (next < ntiles) load_halo(next, IC<0>{}, IC<NHC>{});
      }
      // dgrad, 32 x 32 form: GELU' operands of co tile n for rows m (two 16-B loads per row)
      auto load_sp = [&](int m, int y, int n) __attribute__((always_inline)) {
        const int xs = min(xo, g.W - 1);
#pragma unroll
        for (int pp = 0; pp < 2; ++pp)
          sp[m][n][pp] = *reinterpret_cast<const u32x4*>(S + pix_off32<OUT_D2S>(b, y, xs, g.H, g.W, C) + 32 * n +
                                                         16 * pp + 8 * h);
      };
      // dgrad, 16 x 16 form: the operands of channel group q (32 q .. 32 q + 31) of rows m
      auto load_sp16 = [&](int m, int y, int q) __attribute__((always_inline)) {
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
          const int xs = min(x0 + 16 * pt + l15, g.W - 1);
          sp[m][pt][q] = *reinterpret_cast<const u32x4*>(S + pix_off32<OUT_D2S>(b, y, xs, g.H, g.W, C) + 32 * q +
                                                         16 * (g4 & 1) + 8 * (g4 >> 1));
        }
      };
      if constexpr (OUT_GGRAD && tap == 7) {
        // dgrad: the pre-activation S of this tile's outputs for the GELU' epilogue
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int y = min(y0 + MT * wave + m, g.H - 1);
          if constexpr (M16) {
            load_sp16(m, y, 0);
            if constexpr (SP_AT7) {
#pragma unroll
              for (int q = 1; q < NQ; ++q) load_sp16(m, y, q);
            }
          } else {
            load_sp(m, y, 0);
            if constexpr (SP_AT7) {
#pragma unroll
              for (int q = 1; q < NQ; ++q) load_sp(m, y, q);
            }
          }
        }
      }
      if constexpr (M16) {
        // fragment lane offsets of this tap: X rows 2w + m + dy, pixels dx + 16 pt + l15
        int xq[MT][PT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int pt = 0; pt < PT; ++pt) {
            const int p = opaque((MT * wave + m + dy) * HWD + dx + 16 * pt) + l15;
            xq[m][pt] = v3_slot<C, true>(p, g4);
          }
        // groups (ks, fragment pair) in sequence; the MT * PT X fragments of a k step are numbered
        // PT * m + pt and paired in that order (a row's two pixel tiles, or the two rows of a
        // 16-pixel tile): a group's two X fragments feed 2 NT16 MFMAs, the
        // next group's are read at its start; weight fragments in a ring of two, one co tile
        // ahead (re-read per row m: 16 reads per 24 MFMAs, within the LDS budget of 16x16x32
        // gaps; double-buffering all four X fragments of a k step spilled)
        bf16x8 xb[2][2], wf[2];
        constexpr int GPK = MT * PT / 2;  // groups per k step
        auto read_x = [&](auto GI, int set) __attribute__((always_inline)) {
          constexpr int gi = decltype(GI)::value, ks = gi / GPK, f0 = 2 * (gi % GPK);
#pragma unroll
          for (int j = 0; j < 2; ++j)
            xb[set][j] = *reinterpret_cast<const bf16x8*>(sX + v3_kstep<C>(xq[(f0 + j) / PT][(f0 + j) % PT], ks));
        };
        auto read_w = [&](auto GI, int n) __attribute__((always_inline)) -> bf16x8 {
          constexpr int ks = decltype(GI)::value / GPK;
          return *reinterpret_cast<const bf16x8*>(wcur + 16 * n * C + v3_kstep<C>(wk16, ks));
        };
        read_x(IC<0>{}, 0);
        wf[0] = read_w(IC<0>{}, 0);
        static_for([&](auto GI) {
          constexpr int gi = decltype(GI)::value, f0 = 2 * (gi % GPK);
          constexpr int cur = gi & 1;
          if constexpr (gi + 1 < KS16 * GPK) read_x(IC<gi + 1>{}, cur ^ 1);
          static_for([&](auto NI) {
            constexpr int n = decltype(NI)::value;
            constexpr int j = NT16 * gi + n;  // weight fragment sequence number: register set j & 1
            if constexpr (n < NT16 - 1) wf[(j + 1) & 1] = read_w(IC<gi>{}, n + 1);
            else if constexpr (gi + 1 < KS16 * GPK) wf[(j + 1) & 1] = read_w(IC<gi + 1>{}, 0);
#pragma unroll
            for (int jx = 0; jx < 2; ++jx) {
              const int m = (f0 + jx) / PT, pt = (f0 + jx) % PT;
              if constexpr (MSU_EXP & 128) asm volatile("" ::"v"(wf[j & 1]), "v"(xb[cur][jx]));  // ablation: no MFMA
              else acc4[m][pt][n] = Fmt16<T>::mma16(wf[j & 1], xb[cur][jx], acc4[m][pt][n]);
            }
          }, std::make_integer_sequence<int, NT16>{});
          __builtin_amdgcn_sched_barrier(0);
        }, std::make_integer_sequence<int, KS16 * GPK>{});
      } else {
        // fragment lane offsets of this tap: X rows 2w + m + dy, pixels dx + xl
        // (recomputed per tap through opaque(): hoisted, the nine taps' offsets would pin 36 VGPRs)
        int xo0[MT], xo1[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int p = opaque((MT * wave + m + dy) * HWD + dx) + xl;
          xo0[m] = p * C + koff(v3_swz<C, false>(p), 0);
          xo1[m] = p * C + koff(v3_swz<C, false>(p), 1);
        }
        // X fragments double buffered (k step ks + 1 read before the MFMAs of ks); each weight
        // fragment is read one co tile ahead of its two MFMAs (registers: the halo prefetch
        // holds 60 VGPRs across the taps)
        bf16x8 xa[2][MT], wf[2];
        auto read_x = [&](auto KSI, int set) __attribute__((always_inline)) {
          constexpr int ks = decltype(KSI)::value;
          constexpr int kb = 32 * (ks >> 1);  // elements: 4 chunks per even / odd pair
#pragma unroll
          for (int m = 0; m < MT; ++m)
            xa[set][m] = *reinterpret_cast<const bf16x8*>(sX + ((ks & 1) ? xo1[m] : xo0[m]) + kb);
        };
        auto read_w = [&](auto KSI, int n) __attribute__((always_inline)) -> bf16x8 {
          constexpr int ks = decltype(KSI)::value;
          constexpr int kb = 32 * (ks >> 1);
          return *reinterpret_cast<const bf16x8*>(wcur + 32 * n * C + ((ks & 1) ? wk1 : wk0) + kb);
        };
        read_x(IC<0>{}, 0);
        wf[0] = read_w(IC<0>{}, 0);
        static_for([&](auto KSI) {
          constexpr int ks = decltype(KSI)::value;
          constexpr int cur = ks & 1;
          if constexpr (ks + 1 < KS32) read_x(IC<ks + 1>{}, cur ^ 1);
          static_for([&](auto NI) {
            constexpr int n = decltype(NI)::value;
            constexpr int j = NT32 * ks + n;  // weight fragment sequence number: register set j & 1
            // (reading it two groups ahead in a ring of three measured no faster and spills the dgrad)
            if constexpr (n < NT32 - 1) wf[(j + 1) & 1] = read_w(IC<ks>{}, n + 1);
            else if constexpr (ks + 1 < KS32) wf[(j + 1) & 1] = read_w(IC<ks + 1>{}, 0);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
              if constexpr (MSU_EXP & 128) asm volatile("" ::"v"(wf[j & 1]), "v"(xa[cur][m]));  // ablation: no MFMA
              else acc[m][n] = Fmt16<T>::mma32(wf[j & 1], xa[cur][m], acc[m][n]);
            }
          }, std::make_integer_sequence<int, NT32>{});
          __builtin_amdgcn_sched_barrier(0);
        }, std::make_integer_sequence<int, KS32>{});
      }
      if constexpr (tap == 8) {
        if constexpr (OUT_GGRAD && !SP_AT7) {
          // the other 32-channel groups' GELU' operands after the last MFMAs: held through taps 7-8 beside the
          // full halo prefetch they pushed the kernel past 256 VGPRs (halo registers spilled,
          // each spill store a vmcnt(0) at tap 1); their latency is exposed at the epilogue's
          // wait instead
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const int y = min(y0 + MT * wave + m, g.H - 1);
#pragma unroll
            for (int q = 1; q < NQ; ++q) {
              if constexpr (M16) load_sp16(m, y, q);
              else load_sp(m, y, q);
            }
          }
        }
        if (next < ntiles) {
          __syncthreads();  // every wave's last halo read done (s_barrier + lgkmcnt)
          store_halo();
        }
      }
      wbuf ^= 1;
    }, std::make_integer_sequence<int, 9>{});
    // the epilogue's start: the GELU' operands landed; then the next tile's W(1) DMA (into
    // tap 8's weight buffer: every wave passed tap 8's barrier before the halo store) ahead of
    // this tile's output stores, so tap 1 of the next tile waits for it and not for the stores
    auto epi_start = [&]() __attribute__((always_inline)) {
      // the GELU' operands landed; pinned after the wait (an empty asm redefining them), or the
      // compiler still counts them pending and puts a vmcnt(0) in front of each first use --
      // behind the previous store group's stores
      if constexpr (OUT_GGRAD) {
        wait_vmcnt<0>();
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < (M16 ? PT : NQ); ++n)
#pragma unroll
            for (int pp = 0; pp < (M16 ? NQ : 2); ++pp) vreg_pin(sp[m][n][pp]);
      }
      w1_early = next < ntiles;
      st_full = w1_early && x0 + TWV <= g.W && y0 + TH <= g.H;
      if (w1_early) dma_w(1, wbuf ^ 1);
    };

    if constexpr (M16) {
      // epilogue: lane holds pixel x0 + 16 pt + l15, channels 16n + 4 g4 + r; a permlane16 swap
      // of co tiles (2q, 2q + 1) gives every lane 8 consecutive channels co8 .. co8 + 7 with
      // co8 = 16 (2q + (g4 & 1)) + 8 (g4 >> 1) (lanes l, l ^ 16 share the pixel)
      const int cofs = 16 * (g4 & 1) + 8 * (g4 >> 1);
      float4 bq[NQ][2];
      if constexpr (BIAS) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          bq[q][0] = *reinterpret_cast<const float4*>(sB + 32 * q + cofs);
          bq[q][1] = *reinterpret_cast<const float4*>(sB + 32 * q + cofs + 4);
        }
      }
      epi_start();
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const int px = x0 + 16 * pt + l15;
        if (px >= g.W) continue;  // lanes l and l ^ 16 agree
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          if constexpr (BIAS) {
            const float4 t0 = bq[q][0], t1 = bq[q][1];
            bv[0] = t0.x; bv[1] = t0.y; bv[2] = t0.z; bv[3] = t0.w;
            bv[4] = t1.x; bv[5] = t1.y; bv[6] = t1.z; bv[7] = t1.w;
          }
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const int y = y0 + MT * wave + m;
            float v[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc4[m][pt][2 * q][i]),
                                                              __float_as_uint(acc4[m][pt][2 * q + 1][i]), false, false);
              v[i] = __uint_as_float(r[0]) + bv[i];
              v[4 + i] = __uint_as_float(r[1]) + bv[4 + i];
            }
            if (y >= g.H) continue;
            if constexpr (OUT_GGRAD) {
              const u32x4 t = sp[m][pt][q];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                v[2 * i] *= gelu_grad_fast(Fmt16<T>::lo(t[i]));
                v[2 * i + 1] *= gelu_grad_fast(Fmt16<T>::hi(t[i]));
              }
            }
            const u32x4 pk = {pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7])};
            const int off = pix_off32<OUT_D2S>(b, y, px, g.H, g.W, C) + 32 * q + cofs;
            // ablation: no output stores (results wrong; the never-true test keeps the MFMAs alive)
            if constexpr (MSU_EXP & 64) if (v[0] != 1.2345e-30f) continue;
            *reinterpret_cast<u32x4*>(Y + off) = pk;
            if constexpr (DUAL) *reinterpret_cast<u32x4*>(Y2 + off) = gelu8<T>(pk);
          }
        }
      }
    } else {
    // epilogue: lane holds pixel xo, channels 32n + 8q + 4h + e of rows 2w + m; the
    // permlane32 swap gives lane l < 32 channels 32n + 16pp + 0..7 and l + 32 the next 8
    // bias columns of this lane's 6 store groups, loaded together: one wait, not one per
    // store group behind the previous group's stores
    float4 bq[NT32][2][2];
    if constexpr (BIAS) {
#pragma unroll
      for (int n = 0; n < NT32; ++n)
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
          const int co = 32 * n + 16 * pp + 8 * h;
          bq[n][pp][0] = *reinterpret_cast<const float4*>(sB + co);
          bq[n][pp][1] = *reinterpret_cast<const float4*>(sB + co + 4);
        }
    }
    epi_start();
    if (xo < g.W) {
#pragma unroll
      for (int n = 0; n < NT32; ++n)
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
          const int co = 32 * n + 16 * pp + 8 * h;
          float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          if constexpr (BIAS) {
            const float4 t0 = bq[n][pp][0], t1 = bq[n][pp][1];
            bv[0] = t0.x; bv[1] = t0.y; bv[2] = t0.z; bv[3] = t0.w;
            bv[4] = t1.x; bv[5] = t1.y; bv[6] = t1.z; bv[7] = t1.w;
          }
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const int y = y0 + MT * wave + m;
            float v[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[m][n][8 * pp + i]),
                                                              __float_as_uint(acc[m][n][8 * pp + 4 + i]), false, false);
              v[i] = __uint_as_float(r[0]) + bv[i];
              v[4 + i] = __uint_as_float(r[1]) + bv[4 + i];
            }
            if (y >= g.H) continue;
            if constexpr (OUT_GGRAD) {
              const u32x4 t = sp[m][n][pp];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                v[2 * i] *= gelu_grad_fast(Fmt16<T>::lo(t[i]));
                v[2 * i + 1] *= gelu_grad_fast(Fmt16<T>::hi(t[i]));
              }
            }
            const u32x4 pk = {pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7])};
            const int off = pix_off32<OUT_D2S>(b, y, xo, g.H, g.W, C) + co;
            // ablation: no output stores (results wrong; the never-true test keeps the MFMAs alive)
            if constexpr (MSU_EXP & 64) if (v[0] != 1.2345e-30f) continue;
            *reinterpret_cast<u32x4*>(Y + off) = pk;
            if constexpr (DUAL) *reinterpret_cast<u32x4*>(Y2 + off) = gelu8<T>(pk);
          }
        }
    }
    }
    if (next >= ntiles) break;
    // the next tile's halo (stored after tap 8) visible to every wave before its tap 0
    __syncthreads();
    tile = next;
    next = tq != nullptr ? read_q() : next + (int)gridDim.x;
  }
  finish();
}

// ------------------------------------------------------------------ wgrad kernel
// dW[dy][co][dx][ci] partial per block: sum over the block's pixel tiles of
//   DY[pixel][co] * Xt[pixel + (dy-1, dx-1)][ci];  one block = one dy, NT waves (one per
//   co tile), each wave 3 * CinP/16 n-tiles.  dbias partial from the dy == 0 blocks.

template <typename T, int NT, int NTI, int TH, bool IN_D2S, bool IN_GELU>
__global__ void __launch_bounds__(64 * NT) conv3x3_wgrad_kernel(const T* __restrict__ X,
                                                                const T* __restrict__ DY,
                                                                float* __restrict__ part,
                                                                float* __restrict__ dbpart,
                                                                ConvGeom g, int nchunk) {
  // NT = Cout/16 (waves), NTI = CinP/16 (ci tiles per dx)
  constexpr int NTHR = 64 * NT;
  constexpr int NPIX = TH * TW;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* sX = reinterpret_cast<T*>(smem_raw);         // [TH][TW+2][PS]
  T* sD = sX + TH * (TW + 2) * g.PS;              // [NPIX][PSD]   (PSD = Cout + pad)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int w = xcd_remap(blockIdx.x, gridDim.x);
  const int dy = w % 3, chunk = w / 3;
  const int tiles_x = (g.W + TW - 1) / TW, tiles_y = (g.H + TH - 1) / TH;
  const long ntiles = (long)g.B * tiles_x * tiles_y;

  f32x4 acc[3][NTI];
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int n = 0; n < NTI; ++n) acc[d][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;

  for (long tile = chunk; tile < ntiles; tile += nchunk) {
    const int b = (int)(tile / ((long)tiles_x * tiles_y));
    const int trem = (int)(tile - (long)b * tiles_x * tiles_y);
    const int y0 = (trem / tiles_x) * TH, x0 = (trem % tiles_x) * TW;
    __syncthreads();
    stage_halo<T, IN_D2S, IN_GELU>(X, sX, b, y0 + dy - 1, TH, x0, g, tid, NTHR);
    // dY tile [NPIX][Cout]: rows outside the image are zero
    {
      const int cpp = g.Cout / 8;
      for (int i = tid; i < NPIX * cpp; i += NTHR) {
        const int pix = i / cpp, ch = i - pix * cpp;
        const int y = y0 + pix / TW, x = x0 + pix % TW;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
        if (y < g.H && x < g.W) {
          const T* p = DY + (((long)b * g.H + y) * g.W + x) * g.Cout + ch * 8;
          float a[4], c[4];
          Vec4<T>::load(p, a);
          Vec4<T>::load(p + 4, c);
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = c[e]; }
        }
        float lo[4] = {v[0], v[1], v[2], v[3]}, hi[4] = {v[4], v[5], v[6], v[7]};
        Vec4<T>::store(sD + pix * g.PSD + ch * 8, lo);
        Vec4<T>::store(sD + pix * g.PSD + ch * 8 + 4, hi);
      }
    }
    __syncthreads();
    if (dy == 0 && tid < g.Cout) {
      for (int p = 0; p < NPIX; ++p) dbacc += to_f32(sD[p * g.PSD + tid]);
    }
    auto rowA = [&](int k) { return sD + k * g.PSD; };
#pragma unroll
    for (int ks = 0; ks < NPIX / 32; ++ks) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        auto rowB = [&](int k) { return sX + ((k / TW) * (TW + 2) + (k % TW) + d) * g.PS; };
#pragma unroll
        for (int n = 0; n < NTI; ++n)
          TR<T>::mma(acc[d][n], rowA, wave * 16, rowB, n * 16, ks * 32, lane);
      }
    }
  }
  // partial [blk][dy][co][dx][ci]   (co = wave*16 + row, ci = n*16 + (lane&15))
  float* out = part + ((long)chunk * 3 + dy) * (long)g.Cout * 3 * g.CinP;
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int n = 0; n < NTI; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = wave * 16 + (lane >> 4) * 4 + r;
        const int ci = n * 16 + (lane & 15);
        out[((long)co * 3 + d) * g.CinP + ci] = acc[d][n][r];
      }
  if (dy == 0 && tid < g.Cout) dbpart[(long)chunk * g.Cout + tid] = dbacc;
}

// ------------------------------------------------------------------ 16-bit wgrad, v2
// Persistent weight gradient for CinP = Cout = C (96, 128) on v_mfma_f32_16x16x32.  One
// 12-wave workgroup per CU (3 waves per SIMD) owns the accumulators of all nine taps of COB
// output channels x C input channels for its share of the pixels: wave w = (dy = w/4, co half,
// ci half) holds 3 dx x NI co-tiles x NJ ci-tiles of 16 x 16.  Per pixel tile (4 rows x 32
// pixels) the input halo [(4+2) x 34][C] and the dY tile [128][COB] sit in LDS, each padded to
// an odd number of 16-B slots per pixel (WG2 below); both operands are read k-strided
// (k = pixels) with ds_read_b64_tr_b16.  Staging is LDS-DMA (global_load_lds_dwordx4) into the
// other of two LDS buffers while the current tile is multiplied: the X image and then the dY
// image are filled lane-linearly, slot by slot; pad slots and out-of-image pixels read a 16-B
// zero block.  After its own DMAs land (vmcnt), each wave GELU-converts the halo slots it
// wrote, in place, so no registers are held across the tile and no extra barrier is needed.
//   C = 96: COB = 96, 3 x 3 tiles per dx (108 accumulator registers), both images at a pixel
//   stride of 104 elements (13 slots).  Block s takes the tiles s, s + gridDim.x, ...
//   C = 128: all nine taps of 128 x 128 are 576 KB of f32 accumulators, more than a CU's
//   register file, so a workgroup owns one HALF of the output channels (COB = 64, SPLIT = 2):
//   block 2 s + h takes the tiles of pixel share s (s, s + nshare, ...) and co 64 h .. 64 h + 63,
//   2 x 4 tiles per dx (96 registers); X at a stride of 136 (17 slots), the block's dY half-tile
//   at 72 (9 slots).  Each X band is staged by the two blocks of a share.
// Partials: chunk s of [chunk][dy][co][dx][ci] + db [chunk][co], each block writing its COB co
// rows: the layout colsum_multi sums, deterministically, over nshare chunks.
template <int C_>
struct WG2 {
  static_assert(C_ == 96 || C_ == 128, "widths with a register plan");
  static constexpr int C = C_;
  static constexpr int COB = C == 96 ? 96 : 64, SPLIT = C / COB;  // co per workgroup, workgroups per pixel share
  static constexpr int TH = 4, TWV = 32, NW = 12, HWD = TWV + 2;
  static constexpr int NI = COB / 32, NJ = C / 32;  // 16-wide co / ci tiles per wave
  static constexpr int PSX = C + 8, SLX = PSX / 8;      // X image: pixel stride, 16-B slots per pixel (1 pad)
  static constexpr int PSD = COB + 8, SLD = PSD / 8;    // dY image
  static constexpr int HPIX = (TH + 2) * HWD;    // 204 halo pixels
  static constexpr int DPIX = TH * TWV;          // 128 dY pixels
  static constexpr int XSLOT = HPIX * SLX;       // slots of the X image; the dY image follows
  static constexpr int NSLOT = XSLOT + DPIX * SLD;
  static constexpr int NINS = (NSLOT + 63) / 64;  // DMA wave-instructions per tile
  static constexpr int PER_WAVE = (NINS + NW - 1) / NW;
  static constexpr int BUF = NINS * 64 * 8;      // elements per LDS buffer (covers the overrun)
  static constexpr size_t LDS = 2 * sizeof(bf16_t) * (size_t)BUF;
  static_assert(LDS <= 160 * 1024, "LDS");
  static_assert(2 * ((3 * HWD + 2) * PSX + 16 * (NJ - 1) + 32 * PSX) < 65536 &&
                    2 * (3 * TWV * PSD + 16 * (NI - 1) + 32 * PSD) < 65536 && 2 * 16 * PSD * (DPIX / 16 - 1) < 65536,
                "fragment and bias read offsets are immediates");
  // A half-wave's k-strided read touches the 8 pixels of one parity, 32 B (8 banks) each.  Pixels
  // two apart are PS dwords apart, so the 8 spans are the multiples 0 .. 7 of PS mod 64 banks:
  // all 64 banks once iff PS = 8 * odd (104 = 8 * 13, 136 = 8 * 17, 72 = 8 * 9).
  static_assert(PSX % 16 == 8 && PSD % 16 == 8, "pixels of one parity on distinct 32-B bank spans");
  // slot ch0 of a pixel's sl slots -> its 16-B chunk; the pad slot re-reads chunk 0
  static MSU_DEV int chunk(int ch0, int sl) { return ch0 < sl - 1 ? ch0 : 0; }
};

template <typename T, int C, bool IN_D2S, bool IN_GELU>
__global__ void __launch_bounds__(768) conv3x3_wgrad_v2_kernel(const bf16_t* __restrict__ X,
                                                               const bf16_t* __restrict__ DY,
                                                               float* __restrict__ part,
                                                               float* __restrict__ dbpart, ConvGeom g,
                                                               int ntiles) {
  using G = WG2<C>;
  constexpr int COB = G::COB, SPLIT = G::SPLIT, TH = G::TH, TWV = G::TWV, NW = G::NW, HWD = G::HWD;
  constexpr int NI = G::NI, NJ = G::NJ, PSX = G::PSX, SLX = G::SLX, PSD = G::PSD, SLD = G::SLD;
  constexpr int HPIX = G::HPIX, DPIX = G::DPIX, XSLOT = G::XSLOT, NSLOT = G::NSLOT;
  constexpr int NINS = G::NINS, PER_WAVE = G::PER_WAVE, BUF = G::BUF;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef __attribute__((address_space(1))) void glb_void;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16_t* lds = reinterpret_cast<bf16_t*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dy = wave >> 2, coh = (wave >> 1) & 1, cih = wave & 1;
  const int share = blockIdx.x / SPLIT, half = blockIdx.x % SPLIT, nshare = gridDim.x / SPLIT;
  const int tiles_x = (g.W + TWV - 1) / TWV, tiles_y = (g.H + TH - 1) / TH;
  const int per_img = tiles_x * tiles_y;

  auto coords = [&](int tile, int& b, int& y0, int& x0) {
    b = tile / per_img;
    const int r = tile - b * per_img;
    y0 = (r / tiles_x) * TH;
    x0 = (r - (r / tiles_x) * tiles_x) * TWV;
  };
  // issue this wave's DMAs of tile `tile` into buffer `buf`
  auto stage = [&](int tile, int buf) __attribute__((always_inline)) {
    int b, y0, x0;
    coords(tile, b, y0, x0);
    const int ln = opaque(lane);
#pragma unroll
    for (int r = 0; r < PER_WAVE; ++r) {
      const int k = wave + NW * r;
      if (k < NINS) {
        const int s = 64 * k + ln;
        const void* src = zero_src(s);
        // slot -> (pixel, 16-B chunk) of its image; the pad slot re-reads chunk 0 of the pixel.
        // With one slot count for both images (C = 96) the dY slots continue the X image's
        // pixels: (pix, chx) is worked out once, ahead of the branch, and serves both images
        // (written inside the branches it is done in both: 2113 instead of 2055 instructions in
        // the plain bf16 kernel, r13a).
        constexpr bool ONE = SLD == SLX;
        const int pix = s / SLX, chx = ONE ? G::chunk(s - pix * SLX, SLX) : 0;
        if (ONE ? pix < HPIX : s < XSLOT) {
          const int ch = ONE ? chx : G::chunk(s - pix * SLX, SLX);
          const int row = pix / HWD, col = pix - (pix / HWD) * HWD;
          const int y = y0 - 1 + row, x = x0 - 1 + col;
          if (y >= 0 && y < g.H && x >= 0 && x < g.W) src = X + pix_off32<IN_D2S>(b, y, x, g.H, g.W, C) + ch * 8;
        } else if (ONE ? pix < HPIX + DPIX : s < NSLOT) {
          const int t = s - XSLOT;
          const int dp = ONE ? pix - HPIX : t / SLD;
          const int ch = ONE ? chx : G::chunk(t - dp * SLD, SLD);
          const int y = y0 + dp / TWV, x = x0 + dp % TWV;
          if (y < g.H && x < g.W) src = DY + pix_off32<false>(b, y, x, g.H, g.W, C) + COB * half + ch * 8;
        }
        // ablation 4096: no DMA (the LDS images stay stale; results wrong)
        if constexpr (!(MSU_EXP & 4096))
          __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(lds + buf * BUF + 64 * 8 * k), 16, 0, 0);
      }
    }
  };
  // after this wave's DMAs landed: GELU the halo slots it wrote, in place
  auto gelu_own = [&](int buf) __attribute__((always_inline)) {
    if constexpr (IN_GELU) {
      const int ln = opaque(lane);
#pragma unroll
      for (int r = 0; r < PER_WAVE; ++r) {
        const int k = wave + NW * r;
        const int s = 64 * k + ln;
        if (k < NINS && s < XSLOT && s % SLX < SLX - 1) {
          u32x4* p = reinterpret_cast<u32x4*>(lds + buf * BUF + 8 * s);
          *p = gelu8<T>(*p);
        }
      }
    }
  };

  f32x4 acc[3][NI][NJ];  // [dx][co tile][ci tile]
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[d][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc[2] = {0.f, 0.f};
  // bias gradient: 16 pixel groups x COB / 2 channel pairs (all 768 threads at 96, 512 at 128)
  const bool dbon = 16 * (COB / 2) >= 64 * NW || tid < 16 * (COB / 2);
  const int dbc = 2 * (tid % (COB / 2)), dbg = dbon ? tid / (COB / 2) : 0;

  int tile = share;
  int cur = 0;
  if (tile < ntiles) {
    stage(tile, 0);
    __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) & lgkmcnt(0)
    gelu_own(0);
  }
  __syncthreads();
  for (; tile < ntiles; tile += nshare) {
    const int next = tile + nshare;
    if (next < ntiles) stage(next, cur ^ 1);
    const bf16_t* sX = lds + cur * BUF;
    const bf16_t* sD = sX + HPIX * PSX;
    // All LDS reads of the tile are untracked (inline asm): a compiler-visible ds_read would
    // be preceded by vmcnt(0) for the next tile's pending LDS-DMA and serialise the two.
    // bias gradient: 8 pixels per group and tile (ablation 65536: none)
    if constexpr (!(MSU_EXP & 65536)) {
      const uint32_t ba = lds_u32(sD + dbg * PSD + dbc);
      uint32_t v[DPIX / 16];
      unroll_for<DPIX / 16>([&](auto P) {
        v[decltype(P)::value] = ds_b32_untracked<2 * 16 * PSD * decltype(P)::value>(ba);
      });
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int p = 0; p < DPIX / 16; ++p) {
        vreg_pin(v[p]);
        dbacc[0] += Fmt16<T>::lo(v[p]);
        dbacc[1] += Fmt16<T>::hi(v[p]);
      }
    }
    // lane part of a k-strided fragment read: pixels 2(4g + q) + half (+16 for the second
    // half of the fragment), g = lane group within the 32-lane half, q = (lane&15)>>2,
    // columns 4(lane&3); everything else is an immediate offset.  Same pixel order for both
    // operands; pixels of one parity sit on distinct 32-B bank spans (WG2), so each half's 32
    // lanes hit all 64 banks once (pixels 8(lane>>4) + q: 2-way conflicts).
    const int lpix = 2 * (4 * ((lane >> 4) & 1) + ((lane & 15) >> 2)) + (lane >> 5);
    const int lx = opaque(lpix * PSX + 4 * (lane & 3));
    const int ld = PSD == PSX ? lx : opaque(lpix * PSD + 4 * (lane & 3));
    const uint32_t xa = lds_u32(sX + lx + dy * HWD * PSX + (C / 2) * cih);
    const uint32_t da = lds_u32(sD + ld + (COB / 2) * coh);
    unroll_for<TH>([&](auto R) {
      constexpr int r = decltype(R)::value;
      // the dY fragments of row r serve all three dx (read once per row, not once per dx: at 96
      // 12 instead of 18 fragment reads per 27 MFMAs -- the LDS reads bound this loop).
      // (Reading group g + 1's X fragments before group g's MFMAs measured no faster, r06x:
      // the loop is bound by its operand traffic, ablations r06w.)
      bf16x8 af[NI];
      unroll_for<NI>([&](auto I) {
        constexpr int o = 2 * (r * TWV * PSD + 16 * decltype(I)::value);
        if constexpr (MSU_EXP & 32768) af[decltype(I)::value] = bf16x8{};  // ablation: no fragment reads
        else af[decltype(I)::value] = tr8_untracked<o, o + 32 * PSD>(da);
      });
      unroll_for<3>([&](auto D) {
        constexpr int d = decltype(D)::value;
        bf16x8 bf[NJ];
        unroll_for<NJ>([&](auto J) {
          constexpr int o = 2 * ((r * HWD + d) * PSX + 16 * decltype(J)::value);
          if constexpr (MSU_EXP & 32768) bf[decltype(J)::value] = bf16x8{};
          else bf[decltype(J)::value] = tr8_untracked<o, o + 32 * PSX>(xa);
        });
        lds_wait_tie<0>();
#pragma unroll
        for (int j = 0; j < NJ; ++j) vreg_pin(bf[j]);
        if constexpr (d == 0) {
#pragma unroll
          for (int i = 0; i < NI; ++i) vreg_pin(af[i]);
        }
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            if constexpr (MSU_EXP & 16384) asm volatile("" ::"v"(af[i]), "v"(bf[j]));  // ablation: no MFMA
            else acc[d][i][j] = Fmt16<T>::mma16(af[i], bf[j], acc[d][i][j]);
        __builtin_amdgcn_sched_barrier(0);
      });
    });
    if (next < ntiles) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      gelu_own(cur ^ 1);
    }
    __syncthreads();
    cur ^= 1;
  }
  // partial [share][dy][co][dx][ci]: lane holds co = co0 + 4(lane>>4) + r, ci = ci0 + (lane&15)
  float* out = part + ((long)share * 3 + dy) * (long)C * 3 * C;
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = COB * half + (COB / 2) * coh + 16 * i + 4 * (lane >> 4) + r;
          const int ci = (C / 2) * cih + 16 * j + (lane & 15);
          out[((long)co * 3 + d) * C + ci] = acc[d][i][j][r];
        }
  // bias partial: reduce the 16 pixel groups through LDS
  float* red = reinterpret_cast<float*>(smem_raw);
  __syncthreads();
  if (dbon) {
    red[dbg * COB + dbc] = dbacc[0];
    red[dbg * COB + dbc + 1] = dbacc[1];
  }
  __syncthreads();
  if (tid < COB) {
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) sum += red[q * COB + tid];
    dbpart[(long)share * C + COB * half + tid] = sum;
  }
}

// chunk-summed partial [dy][co][dx][ci] -> dW[co][ci][3][3] (torch Conv2d layout)
__global__ void __launch_bounds__(256) wgrad_permute_kernel(const float* __restrict__ sum, int Cout, int Cin,
                                                            int CinP, float* __restrict__ dW, int accumulate) {
  const long n = (long)Cout * Cin * 9;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int co = (int)(i / (Cin * 9));
    const int rem = (int)(i - (long)co * Cin * 9);
    const int ci = rem / 9, tap = rem % 9, dy = tap / 3, dx = tap % 3;
    const float v = sum[((long)dy * Cout * 3 + (long)co * 3 + dx) * CinP + ci];
    dW[i] = accumulate ? dW[i] + v : v;
  }
}

// ------------------------------------------------------------------ host dispatch
ConvGeom make_geom(int B, int H, int W, int Cin, int Cout, int elem_bytes) {
  ConvGeom g;
  g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout;
  g.CinP = (Cin + 31) / 32 * 32;
  const int pad = elem_bytes == 2 ? 8 : 4;
  g.PS = g.CinP + pad;
  g.PSW = g.CinP + pad;
  g.PSD = Cout + pad;
  return g;
}

template <typename T, int NT, bool IN_D2S, bool IN_GELU, bool OUT_D2S, bool OUT_GGRAD, bool BIAS, bool DUAL>
int launch_conv(const ConvGeom& g, const T* X, const T* Wt, const float* bias, const T* S, T* Y, T* Y2,
                hipStream_t st) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int TH = BF ? 16 : 4;
  constexpr int MT = BF ? 2 : 1;
  constexpr int NW = TH / MT;
  const size_t lds = sizeof(T) * ((size_t)(TH + 2) * (TW + 2) * g.PS + (size_t)(BF ? 2 : 1) * g.Cout * g.PSW);
  if (lds > 160 * 1024) return -4;
  auto kern = conv3x3_kernel<T, NT, TH, MT, BF, IN_D2S, IN_GELU, OUT_D2S, OUT_GGRAD, BIAS, DUAL>;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  const long ntiles = (long)g.B * ((g.W + TW - 1) / TW) * ((g.H + TH - 1) / TH);
  if (ntiles == 0) return 0;
  hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(64 * NW), lds, st, X, Wt, bias, S, Y, Y2, g);
  return MSU_CHECK_LAUNCH();
}

// The width of the persistent LDS-DMA kernels (conv3x3_v3_kernel, conv3x3_wgrad_v2_kernel) that
// serves 16-bit Cin -> Cout, or 0: the generic kernels.  The one routing rule of both
// translation units; generic_wide is msu_conv_mode bit 1 (msu_conv3x3_route passes false: it
// reports what is built).  conv3x3_v3_kernel has no GELU on load: those forms stay generic.
inline int persistent_width(bool is16, int Cin, int Cout, bool generic_wide) {
  if (!is16 || Cin != Cout) return 0;
  if (Cin == 96) return 96;
  return Cin == 128 && !generic_wide ? 128 : 0;
}

// msu_conv3x3_route: bit 0 the forward / backward-data launches, bit 1 the weight gradient.
inline int conv_route(bool is16, int Cin, int Cout) { return persistent_width(is16, Cin, Cout, false) ? 3 : 0; }

template <typename T, int C, bool IN_D2S, bool OUT_D2S, bool OUT_GGRAD, bool BIAS, bool DUAL>
int launch_v3(const ConvGeom& g, const bf16_t* X, const bf16_t* Wt, const float* bias, const bf16_t* S, bf16_t* Y,
              bf16_t* Y2, hipStream_t st) {
  // C = 96: forward launches on 16x16x32 MFMA (same tile, LDS images and schedule; (p >> 1) & 3
  // swizzle), since round 4: same-box kbench (r04b) conv1 2.22-2.28 vs 2.44 ms, conv2 1.48 vs
  // 1.55 ms (bare MFMA loops of this shape run at ~1.12-1.15x the FLOP/s of 32x32x16 on MI355X at
  // equal cycles: the clock it holds, MI355X_MICROARCH.md).  The dgrad keeps 32x32x16: with its
  // GELU' operands held from tap 7 the 16x16 form spills 260 B per lane.  Halo loads spread over
  // taps 1..7 (SPREAD; all at tap 1 measured equal, r03).  v4 (one wave per SIMD, 4 rows per
  // wave) was 7-10 % slower on every launch (r03l/m) and is gone.
  // C = 128 (Swin-B decoder head): 8-row tiles, every launch on 16x16x32 MFMA -- with one row per
  // wave only that shape lets a weight fragment feed two MFMAs, and the dgrad's accumulators (64)
  // and GELU' operands (32 registers) are fewer than at 96, so it does not spill there.
  // (ablation 2048: the C = 96 dgrad on 16 x 16 x 32 too; ablation 8192: C = 128 on the 16-row x
  // 16-pixel geometry, two rows per wave)
  constexpr bool M16 = !(C == 96 && OUT_GGRAD) || (MSU_EXP & 2048) != 0;
  constexpr int TWW = (C == 128 && (MSU_EXP & 8192) != 0) ? 16 : 32;
  using G = V3W<C, TWW>;
  constexpr size_t lds = G::LDS;
  auto kern = conv3x3_v3_kernel<T, IN_D2S, OUT_D2S, OUT_GGRAD, BIAS, DUAL, true, M16, C, TWW>;
  const long ntiles = (long)g.B * ((g.W + G::TWV - 1) / G::TWV) * ((g.H + G::TH - 1) / G::TH);
  if (ntiles == 0) return 0;
  // 32-bit element offsets and tile indices inside the kernel (checked before any HIP call)
  if ((long)g.B * g.H * g.W * C >= (1L << 31)) return -2;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  const int grid = (int)(ntiles < msu_num_cus() ? ntiles : msu_num_cus());
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * G::NW), lds, st, X, Wt, bias, S, Y, Y2, g, (int)ntiles,
                     g_conv_dyn ? tile_queue(st) : nullptr);
  return MSU_CHECK_LAUNCH();
}

// persistent width ? launch_v3<C> : the generic kernel by output width
template <typename T, bool IN_D2S, bool IN_GELU, bool OUT_D2S, bool OUT_GGRAD, bool BIAS, bool DUAL = false>
int conv_nt(const ConvGeom& g, const void* X, const void* Wt, const float* bias, const void* S,
            void* Y, void* Y2, hipStream_t st) {
  const T* x = (const T*)X; const T* w = (const T*)Wt; const T* s = (const T*)S; T* y = (T*)Y; T* y2 = (T*)Y2;
  if constexpr (sizeof(T) == 2 && !IN_GELU) {
    auto v3 = [&](auto C) {
      return launch_v3<T, decltype(C)::value, IN_D2S, OUT_D2S, OUT_GGRAD, BIAS, DUAL>(
          g, (const bf16_t*)x, (const bf16_t*)w, bias, (const bf16_t*)s, (bf16_t*)y, (bf16_t*)y2, st);
    };
    switch (persistent_width(true, g.Cin, g.Cout, g_conv_generic_wide != 0)) {
      case 96: return v3(IC<96>{});
      case 128: return v3(IC<128>{});
    }
  }
  switch (g.Cout / 16) {
    case 1: return launch_conv<T, 1, IN_D2S, IN_GELU, OUT_D2S, OUT_GGRAD, BIAS, DUAL>(g, x, w, bias, s, y, y2, st);
    case 2: return launch_conv<T, 2, IN_D2S, IN_GELU, OUT_D2S, OUT_GGRAD, BIAS, DUAL>(g, x, w, bias, s, y, y2, st);
    case 4: return launch_conv<T, 4, IN_D2S, IN_GELU, OUT_D2S, OUT_GGRAD, BIAS, DUAL>(g, x, w, bias, s, y, y2, st);
    case 6: return launch_conv<T, 6, IN_D2S, IN_GELU, OUT_D2S, OUT_GGRAD, BIAS, DUAL>(g, x, w, bias, s, y, y2, st);
    case 8: return launch_conv<T, 8, IN_D2S, IN_GELU, OUT_D2S, OUT_GGRAD, BIAS, DUAL>(g, x, w, bias, s, y, y2, st);
  }
  return -2;
}

template <typename T, int NT, bool IN_D2S, bool IN_GELU>
int launch_wgrad_nti(const ConvGeom& g, const T* X, const T* DY, float* part, float* dbpart,
                     int nchunk, hipStream_t st) {
  constexpr int TH = 8;
  const size_t lds = sizeof(T) * ((size_t)TH * (TW + 2) * g.PS + (size_t)TH * TW * g.PSD);
  if (lds > 160 * 1024) return -4;
  auto go = [&](auto kern) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(kern, dim3((unsigned)(nchunk * 3)), dim3(64 * NT), lds, st, X, DY, part, dbpart, g, nchunk);
    return MSU_CHECK_LAUNCH();
  };
  switch (g.CinP / 16) {
    case 2: return go(conv3x3_wgrad_kernel<T, NT, 2, TH, IN_D2S, IN_GELU>);
    case 4: return go(conv3x3_wgrad_kernel<T, NT, 4, TH, IN_D2S, IN_GELU>);
    case 6: return go(conv3x3_wgrad_kernel<T, NT, 6, TH, IN_D2S, IN_GELU>);
    case 8: return go(conv3x3_wgrad_kernel<T, NT, 8, TH, IN_D2S, IN_GELU>);
  }
  return -2;
}

// Blocks SPLIT s + h = (pixel share s, co part h); nchunk / SPLIT shares, so the grid stays nchunk
// workgroups.  Returns the number of partial chunks written (> 0) or an error (< 0).
template <typename T, int C, bool IN_D2S, bool IN_GELU>
int launch_wgrad_v2(const ConvGeom& g, const bf16_t* X, const bf16_t* DY, float* part, float* dbpart,
                    int nchunk, hipStream_t st) {
  using G = WG2<C>;
  // 32-bit element offsets inside the kernel (checked before any HIP call)
  if ((long)g.B * g.H * g.W * C >= (1L << 31)) return -2;
  auto kern = conv3x3_wgrad_v2_kernel<T, C, IN_D2S, IN_GELU>;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS);
    attr_set = true;
  }
  const int nshare = nchunk >= G::SPLIT ? nchunk / G::SPLIT : 1;
  const long ntiles = (long)g.B * ((g.W + G::TWV - 1) / G::TWV) * ((g.H + G::TH - 1) / G::TH);
  // every block writes its partial rows, even with no tile (zeros)
  hipLaunchKernelGGL(kern, dim3((unsigned)(G::SPLIT * nshare)), dim3(64 * G::NW), G::LDS, st, X, DY, part, dbpart, g,
                     (int)ntiles);
  return MSU_CHECK_LAUNCH() ? -1 : nshare;
}

template <typename T, bool IN_D2S, bool IN_GELU>
int wgrad_nt(const ConvGeom& g, const void* X, const void* DY, float* part, float* dbpart,
             int nchunk, hipStream_t st) {
  const T* x = (const T*)X; const T* d = (const T*)DY;
  switch (g.Cout / 16) {
    case 1: return launch_wgrad_nti<T, 1, IN_D2S, IN_GELU>(g, x, d, part, dbpart, nchunk, st);
    case 2: return launch_wgrad_nti<T, 2, IN_D2S, IN_GELU>(g, x, d, part, dbpart, nchunk, st);
    case 4: return launch_wgrad_nti<T, 4, IN_D2S, IN_GELU>(g, x, d, part, dbpart, nchunk, st);
    case 6: return launch_wgrad_nti<T, 6, IN_D2S, IN_GELU>(g, x, d, part, dbpart, nchunk, st);
    case 8: return launch_wgrad_nti<T, 8, IN_D2S, IN_GELU>(g, x, d, part, dbpart, nchunk, st);
  }
  return -2;
}

}  // namespace

