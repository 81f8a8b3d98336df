// Stage-0 Swin MLP forward in ONE kernel (torchvision MLP, model_parts.py:538):
//
//   y = mlp.3(GELU(mlp.0(x)))      x, y: [M][96], hidden 384
//
// Without autograd (the reference's discarded branches layers_cent1[-1] / layers_cent2[-1] at
// model_parts.py:795 / :807, and evaluation) the 384-wide hidden activation never leaves the
// chip: the GEMM pair wrote GELU(H) (403 MB at 8 x 256^2 tokens) and read it back.  In training
// (H_OUT) the kernel also stores the pre-activation H -- the one tensor the backward needs (mlp.3's
// input gradient applies GELU'(H), its weight gradient re-derives GELU(H) from H while staging:
// msu_linear_bwd with X = null); the pair wrote H and GELU(H) and read GELU(H) back.
// Per 32-token tile and per 32-wide hidden chunk a wave runs
//   * fc1 on MFMA with W1 as the A operand and the tile's token rows as B (the tokens end up on
//     the accumulator columns, the hidden units on its rows), + b1, rounded to 16 bits, GELU
//     (the unfused epilogue's arithmetic: gelu_fast of the rounded pre-activation), rounded
//     again and packed -- each lane's 16 values are directly the B operand of
//   * fc2 (y^T += W2[:, chunk] . G^T[chunk, :]), whose A fragments are read from W2 rows in the
//     accumulator's row order (two 8-B pieces per fragment), three 32-channel output tiles.
// W1 [384][96] (16-B chunks swizzled c ^ ((r >> 2) & 3): conflict-free 32-row fragment reads)
// and W2 [96][388] (194-dword rows: the 32 rows of a ds_read_b64 half-wave fill the 64 banks
// once) stay in LDS for the workgroup's life; the token rows come from HBM straight into
// registers one tile ahead.  One 8-wave workgroup per CU (150 KB of LDS), two waves per SIMD:
// the GELU of one overlaps the other's MFMAs.
#include "common.h"

namespace {

constexpr int MC = 96, MH = 384, MT = 32, MW = 8;
constexpr int LW2 = MH + 4;

struct MlpLds {
  bf16_t w1[MH * MC];
  bf16_t w2[MC * LW2];
  float b1[MH];
  float b2[MC];
  float g2[MC], be2[MC];  // LN_IN: norm2's weight / bias
};

struct MlpArgs {
  const bf16_t* x;      // the MLP input rows; LN_IN: the residual stream a
  const bf16_t* br;     // LN_IN: the branch added to it, scaled per sample
  const float* bscale;  // LN_IN: per-sample scale (StochasticDepth 'row'), null = 1
  long rps;             // LN_IN: rows per sample
  const float* g2;      // LN_IN: norm2 weight / bias, eps
  const float* be2;
  float eps;
  bf16_t* s_out;        // LN_IN: s = a + scale * br (the residual stream the block passes on)
  const bf16_t* w1;
  const float* b1;
  const bf16_t* w2;
  const float* b2;
  bf16_t* y;
  bf16_t* hout;         // H_OUT: the pre-activation
  long M;
};

MSU_DEV int w1_swz(int r) { return (r >> 2) & 3; }

// accumulator row of register r for lane half h (32x32 C layout)
MSU_DEV constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// LN_IN (no-grad blocks): the input rows are LN2(a + scale * br), computed here as the residual-add
// LayerNorm kernel does (the sum rounded to 16 bits and stored as s, two-pass variance), so the
// normalised rows never reach HBM either
template <typename T, bool H_OUT, bool LN_IN>
__global__ void __launch_bounds__(64 * MW) mlp_fused_kernel(MlpArgs A) {
  const bf16_t* __restrict__ x = A.x;
  const bf16_t* __restrict__ w1 = A.w1;
  const float* __restrict__ b1 = A.b1;
  const bf16_t* __restrict__ w2 = A.w2;
  const float* __restrict__ b2 = A.b2;
  bf16_t* __restrict__ y = A.y;
  bf16_t* __restrict__ hout = A.hout;
  const long M = A.M;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  MlpLds& L = *reinterpret_cast<MlpLds*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int s = tid; s < MH * (MC / 8); s += 64 * MW) {
    const int r = s / (MC / 8), c = s % (MC / 8);
    *reinterpret_cast<u32x4*>(L.w1 + r * MC + ((c ^ w1_swz(r)) << 3)) = *reinterpret_cast<const u32x4*>(w1 + r * MC + 8 * c);
  }
  for (int s = tid; s < MC * (MH / 8); s += 64 * MW) {
    const int r = s / (MH / 8), c = s % (MH / 8);
    const u32x4 v = *reinterpret_cast<const u32x4*>(w2 + r * MH + 8 * c);
    // 8-B aligned rows (388 elements): two 8-B stores
    *reinterpret_cast<u32x2*>(L.w2 + r * LW2 + 8 * c) = u32x2{v.x, v.y};
    *reinterpret_cast<u32x2*>(L.w2 + r * LW2 + 8 * c + 4) = u32x2{v.z, v.w};
  }
  for (int s = tid; s < MH; s += 64 * MW) L.b1[s] = b1[s];
  for (int s = tid; s < MC; s += 64 * MW) L.b2[s] = b2[s];
  if constexpr (LN_IN) {
    for (int s = tid; s < MC; s += 64 * MW) {
      L.g2[s] = A.g2[s];
      L.be2[s] = A.be2[s];
    }
  }
  __syncthreads();

  const long ntiles = (M + MT - 1) / MT;
  const long stride = (long)gridDim.x * MW;
  long tile = (long)blockIdx.x * MW + wave;
  if (tile >= ntiles) return;  // no block-wide barriers after this point
  const int tl = lane & 31;
  // token rows of a tile as the fc1 B operand: lane (token tl, half hh) holds k = 16 ks + 8 hh .. + 7
  auto load_x = [&](long t, u32x4 (&xr)[6]) __attribute__((always_inline)) {
    const long row = t * MT + tl;
    const bool ok = row < M;
    const bf16_t* p = x + (ok ? row : 0) * MC + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(p + 16 * ks);
      xr[ks] = ok ? v : u32x4{0u, 0u, 0u, 0u};
    }
  };
  // LN_IN: the branch rows of a tile and their per-sample scale (loaded at the tile's start, not
  // a tile ahead: the registers for a second prefetched set spilled)
  auto load_br = [&](long t, u32x4 (&ar)[6], float& sc) __attribute__((always_inline)) {
    const long row = t * MT + tl;
    const bool ok = row < M;
    const bf16_t* q = A.br + (ok ? row : 0) * MC + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(q + 16 * ks);
      ar[ks] = ok ? v : u32x4{0u, 0u, 0u, 0u};
    }
    sc = A.bscale ? A.bscale[(ok ? row : 0) / A.rps] : 1.f;
  };
  // LN_IN: s = round16(a + sc br) (stored), rows normalised over the token's 96 channels (this
  // lane's 48 and its xor-32 partner's) -> the fc1 B operand
  auto ln_rows = [&](long t, u32x4 (&xr)[6], const u32x4 (&ar)[6], float sc) __attribute__((always_inline)) {
    const long row = t * MT + tl;
    const bool ok = row < M;
    // s = round16(a + sc br), kept packed in xr (the 16-bit values the sums and the output use)
#pragma unroll
    for (int ks = 0; ks < 6; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        xr[ks][i] = pack2<T>(fmaf(sc, Fmt16<T>::lo(ar[ks][i]), Fmt16<T>::lo(xr[ks][i])),
                             fmaf(sc, Fmt16<T>::hi(ar[ks][i]), Fmt16<T>::hi(xr[ks][i])));
    float sum = 0.f;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i) sum += Fmt16<T>::lo(xr[ks][i]) + Fmt16<T>::hi(xr[ks][i]);
    sum += __shfl_xor(sum, 32, 64);
    const float mu = sum / MC;
    float var = 0.f;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d0 = Fmt16<T>::lo(xr[ks][i]) - mu, d1 = Fmt16<T>::hi(xr[ks][i]) - mu;
        var += d0 * d0;
        var += d1 * d1;
      }
    var += __shfl_xor(var, 32, 64);
    const float rs = rsqrtf(var / MC + A.eps);
    bf16_t* srow = A.s_out + (ok ? row : 0) * MC + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      if (ok) *reinterpret_cast<u32x4*>(srow + 16 * ks) = xr[ks];
      const float4 g0 = *reinterpret_cast<const float4*>(L.g2 + 16 * ks + 8 * hh);
      const float4 g1 = *reinterpret_cast<const float4*>(L.g2 + 16 * ks + 8 * hh + 4);
      const float4 c0 = *reinterpret_cast<const float4*>(L.be2 + 16 * ks + 8 * hh);
      const float4 c1 = *reinterpret_cast<const float4*>(L.be2 + 16 * ks + 8 * hh + 4);
      const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      const float bb[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      uint32_t o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[i] = pack2<T>((Fmt16<T>::lo(xr[ks][i]) - mu) * rs * g[2 * i] + bb[2 * i],
                        (Fmt16<T>::hi(xr[ks][i]) - mu) * rs * g[2 * i + 1] + bb[2 * i + 1]);
      xr[ks] = u32x4{o[0], o[1], o[2], o[3]};
      __builtin_amdgcn_sched_barrier(0);  // gamma / beta reads one chunk at a time (hoisted, they spilled)
    }
  };
  u32x4 xc[6], xn[6], ac[6];
  float scc = 1.f;
  load_x(tile, xc);
  // fc2 A fragment of output tile ct, hidden k step n0 .. n0 + 15 in the accumulator row order:
  // element e of half hh <-> hidden n0 + 8 (e >> 2) + 4 hh + (e & 3)
  const bf16_t* w2row = L.w2 + tl * LW2 + 4 * hh;
  for (;;) {
    const long nxt = tile + stride;
    const bool more = nxt < ntiles;
    if constexpr (LN_IN) load_br(tile, ac, scc);
    if (more) load_x(nxt, xn);
    if constexpr (LN_IN) ln_rows(tile, xc, ac, scc);
    f32x16 yacc[3];
#pragma unroll
    for (int ct = 0; ct < 3; ++ct) yacc[ct] = f32x16{0};
    const long hrow_i = tile * MT + tl;
    const bool hok = hrow_i < M;
    bf16_t* hrow = H_OUT ? hout + (hok ? hrow_i : 0) * MH : nullptr;
#pragma unroll((H_OUT || LN_IN) ? 1 : 2)
    for (int nc = 0; nc < MH / 32; ++nc) {
      // fc1: C1^T[n][t] for hidden n in chunk nc
      f32x16 h = f32x16{0};
      const int wr = nc * 32 + tl;
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        const bf16x8 wf = *reinterpret_cast<const bf16x8*>(L.w1 + wr * MC + (((2 * ks + hh) ^ w1_swz(wr)) << 3));
        h = Fmt16<T>::mma32(wf, __builtin_bit_cast(bf16x8, xc[ks]), h);
      }
      // + b1, 16-bit pre-activation, GELU, 16-bit activation (the unfused epilogues' roundings)
      uint32_t g[8], hw[8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 bq = *reinterpret_cast<const float4*>(L.b1 + nc * 32 + 8 * q + 4 * hh);
        const float u0 = round16<T>(h[4 * q] + bq.x), u1 = round16<T>(h[4 * q + 1] + bq.y);
        const float u2 = round16<T>(h[4 * q + 2] + bq.z), u3 = round16<T>(h[4 * q + 3] + bq.w);
        if constexpr (H_OUT) {
          hw[2 * q] = pack2<T>(u0, u1);
          hw[2 * q + 1] = pack2<T>(u2, u3);
        }
        g[2 * q] = pack2<T>(gelu_fast(u0), gelu_fast(u1));
        g[2 * q + 1] = pack2<T>(gelu_fast(u2), gelu_fast(u3));
      }
      if constexpr (H_OUT) {
        // H row piece: a permlane32 swap pairs the halves' 4-unit groups into 8 consecutive
        // hidden units per lane (hidden nc*32 + 16p + 8hh .. + 7), one 16-B store each
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const auto s0 = __builtin_amdgcn_permlane32_swap(hw[4 * p], hw[4 * p + 2], false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(hw[4 * p + 1], hw[4 * p + 3], false, false);
          const u32x4 v = {s0[0], s1[0], s0[1], s1[1]};
          if (hok) *reinterpret_cast<u32x4*>(hrow + nc * 32 + 16 * p + 8 * hh) = v;
        }
      }
      // fc2: two 16-deep k steps over the chunk (registers 8s .. 8s + 7 of the fc1 accumulator)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 gb = __builtin_bit_cast(bf16x8, u32x4{g[4 * s], g[4 * s + 1], g[4 * s + 2], g[4 * s + 3]});
        const int n0 = nc * 32 + 16 * s;
#pragma unroll
        for (int ct = 0; ct < 3; ++ct) {
          const bf16_t* a = w2row + ct * 32 * LW2 + n0;
          const u32x2 lo = *reinterpret_cast<const u32x2*>(a);
          const u32x2 hi = *reinterpret_cast<const u32x2*>(a + 8);
          const bf16x8 af = __builtin_bit_cast(bf16x8, u32x4{lo.x, lo.y, hi.x, hi.y});
          yacc[ct] = Fmt16<T>::mma32(af, gb, yacc[ct]);
        }
      }
    }
    // y[t][c] = y^T + b2: lane (token tl) holds channels 32 ct + 8 q + 4 hh + i in register 4q + i;
    // a permlane32 swap pairs the halves' 4-channel groups into 8 consecutive channels per
    // lane, so every store is one 16-B piece (every lane executes the swaps)
    const long row = tile * MT + tl;
    const bool ok = row < M;
    bf16_t* yr = y + (ok ? row : 0) * MC;
#pragma unroll
    for (int ct = 0; ct < 3; ++ct) {
      uint32_t w[8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 bq = *reinterpret_cast<const float4*>(L.b2 + ct * 32 + 8 * q + 4 * hh);
        w[2 * q] = pack2<T>(yacc[ct][4 * q] + bq.x, yacc[ct][4 * q + 1] + bq.y);
        w[2 * q + 1] = pack2<T>(yacc[ct][4 * q + 2] + bq.z, yacc[ct][4 * q + 3] + bq.w);
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const auto s0 = __builtin_amdgcn_permlane32_swap(w[4 * p], w[4 * p + 2], false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(w[4 * p + 1], w[4 * p + 3], false, false);
        const u32x4 v = {s0[0], s1[0], s0[1], s1[1]};
        if (ok) *reinterpret_cast<u32x4*>(yr + ct * 32 + 16 * p + 8 * hh) = v;
      }
    }
    if (!more) break;
    tile = nxt;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) xc[ks] = xn[ks];
  }
}

template <typename T, bool H_OUT, bool LN_IN = false>
int launch_mlp(const MlpArgs& a, hipStream_t st) {
  auto kern = mlp_fused_kernel<T, H_OUT, LN_IN>;
  const long M = a.M;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(MlpLds)) !=
        hipSuccess)
      return -4;
    attr_set = true;
  }
  const long ntiles = (M + MT - 1) / MT;
  long grid = msu_num_cus();
  if (grid * MW > ntiles) grid = (ntiles + MW - 1) / MW;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * MW), sizeof(MlpLds), st, a);
  return MSU_CHECK_LAUNCH();
}

}  // namespace

// mlp_s1.hip: the streamed-weight form (weights through an LDS ring; hidden 4 C) and its widths
// (C = 192: Swin-T/S stage 1; C = 128 / 256: Swin-B stages 0 / 1)
int msu_mlp_s1_width(int C);
int msu_mlp_s1_launch(int dtype, const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                      void* y, void* h, long M, int C, void* stream);

extern "C" {

// Whether msu_mlp_fused_fwd covers a (channels, hidden) shape: the Swin-T/S stage-0 MLP,
// 96 -> 384 -> 96, its stage-1 MLP, 192 -> 768 -> 192, and the Swin-B stage-0 and stage-1 MLPs,
// 128 -> 512 -> 128 and 256 -> 1024 -> 256 (msu_add_ln_mlp_fwd: 96 -> 384 only).
int msu_mlp_fused_supported(int C, int Hd) {
  return (C == MC && Hd == MH) || (msu_mlp_s1_width(C) && Hd == 4 * C) ? 1 : 0;
}

// y = fc2(GELU(fc1(x))) with the hidden activation kept on chip; h (nullable) receives the
// 16-bit pre-activation fc1(x) [M][Hd] for the backward.  dtype bf16 / f16; x, y [M][C] (16-B
// aligned rows), w1 [Hd][C], w2 [C][Hd] in x's format, b1 [Hd] / b2 [C] f32; (C, Hd) = (96, 384),
// (192, 768), (128, 512) or (256, 1024).
int msu_mlp_fused_fwd(int dtype, const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                      void* y, void* h, long M, int C, int Hd, void* stream) {
  if (!msu_is16(dtype) || !msu_mlp_fused_supported(C, Hd) || M < 0) return -2;
  if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)h | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)b1 | (uintptr_t)b2) &
       15) != 0)
    return -2;
  if (M == 0) return 0;
  if (C != MC) return msu_mlp_s1_launch(dtype, x, w1, b1, w2, b2, y, h, M, C, stream);
  hipStream_t st = (hipStream_t)stream;
  MlpArgs a{};
  a.x = (const bf16_t*)x;
  a.w1 = (const bf16_t*)w1;
  a.b1 = b1;
  a.w2 = (const bf16_t*)w2;
  a.b2 = b2;
  a.y = (bf16_t*)y;
  a.hout = (bf16_t*)h;
  a.M = M;
  if (h != nullptr) {
    MSU_DISPATCH16(dtype, T, return launch_mlp<T, true>(a, st));
  } else {
    MSU_DISPATCH16(dtype, T, return launch_mlp<T, false>(a, st));
  }
  return -3;
}

// No-grad second half of a stage-0 Swin block in one kernel: s = a + bscale[sample] * br
// (rounded to 16 bits; bscale null = 1), y = mlp(LN2(s)) -- msu_layernorm_fwd's residual-add mode
// followed by msu_mlp_fused_fwd, without the normalised rows in HBM.  a, br, s_out, y [M][96];
// rows_per_sample splits the rows into samples for bscale; gamma / beta / eps of norm2.
int msu_add_ln_mlp_fwd(int dtype, const void* a, const void* br, const float* bscale, long rows_per_sample,
                       const float* gamma, const float* beta, float eps, const void* w1, const float* b1,
                       const void* w2, const float* b2, void* s_out, void* y, long M, int C, int Hd, void* stream) {
  if (!msu_is16(dtype) || C != MC || Hd != MH || M < 0 || rows_per_sample <= 0) return -2;
  if ((((uintptr_t)a | (uintptr_t)br | (uintptr_t)s_out | (uintptr_t)y | (uintptr_t)w1 | (uintptr_t)w2 |
        (uintptr_t)b1 | (uintptr_t)b2 | (uintptr_t)gamma | (uintptr_t)beta) & 15) != 0)
    return -2;
  if (M == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  MlpArgs p{};
  p.x = (const bf16_t*)a;
  p.br = (const bf16_t*)br;
  p.bscale = bscale;
  p.rps = rows_per_sample;
  p.g2 = gamma;
  p.be2 = beta;
  p.eps = eps;
  p.s_out = (bf16_t*)s_out;
  p.w1 = (const bf16_t*)w1;
  p.b1 = b1;
  p.w2 = (const bf16_t*)w2;
  p.b2 = b2;
  p.y = (bf16_t*)y;
  p.M = M;
  MSU_DISPATCH16(dtype, T, return (launch_mlp<T, false, true>(p, st)));
  return -3;
}

}  // extern "C"
