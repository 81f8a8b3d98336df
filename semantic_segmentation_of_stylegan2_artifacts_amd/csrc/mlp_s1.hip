// Swin MLP forward in ONE kernel with the weights streamed through LDS (torchvision MLP,
// model_parts.py:538), a template over the width C (S1W<C> below):
//
//   y = mlp.3(GELU(mlp.0(x)))      x, y: [M][C], hidden 4 C
//
// built for C = 192 (Swin-T/S stage 1, hidden 768), C = 128 (Swin-B stage 0, hidden 512) and, as
// a kernel of its own on the same ring, C = 256 (Swin-B stage 1, hidden 1024: the end of this comment).
// The GEMM pair this replaces wrote H and GELU(H) (2 x 201 MB at C = 192, 8 x 128^2 tokens;
// 2 x 537 MB at C = 128, 8 x 256^2) and read GELU(H) back; here the training form writes H only
// (the backward's GELU' operand) and GELU(H) never leaves the chip.  Unlike the 96 -> 384 kernel
// (mlp_fused.hip) the weights (2 x 8 C^2 bytes: 295 KB / 131 KB each) do not fit one CU's LDS
// beside a ring, so they are STREAMED: the hidden dimension is cut into NU = 4 C / 32 chunks of
// 32 units, each chunk's W1 rows [32][C] and W2 columns [C][32] (128 C bytes: 24 KB / 16 KB) go
// global -> LDS by LDS-DMA into a ring of NS slots (6 / 8), and the workgroup's waves walk the
// chunks in step with one barrier per chunk (interval j refills chunk j - 2's slot with chunk
// j + NS - 2).  The ring runs across the workgroup's token tiles as one flat chunk sequence.
//
// Per wave: a 32-token tile (workgroup: 8 waves, 256 tokens).  The tile's x rows stay in registers
// as fc1's B operand (K1 = C / 16 k steps, C / 4 registers); per chunk
//   * fc1 on MFMA (K1 MFMAs; W1 rows as A, tokens on the accumulator columns), + b1, rounded to
//     16 bits (stored as H), GELU, rounded again: the unfused epilogues' arithmetic;
//   * the packed GELU(H) registers are directly fc2's B operand: the chunk's W1 rows sit in the
//     slot PERMUTED (slot row rho holds hidden unit pi(rho), pi swapping bits 2 and 3), so that
//     accumulator registers 8s .. 8s + 7 of lane half hh hold hidden units 16s + 8hh .. + 7 --
//     consecutive, i.e. ONE 16-B W2 fragment read per fc2 MFMA and one 16-B H store per 8 units;
//   * fc2 (2 NCT MFMAs) accumulates y^T (NCT = C / 32 32-channel tiles, C / 2 registers: 96 / 64)
//     over the NU chunks.
// Slot images: W1 rows 2 C bytes with 16-B column c at c ^ w1_swz(rho) (C = 192: (rho >> 1) & 7;
// C = 128: rho & 15), W2 rows 64 B with column c at c ^ ((row >> 2) & 3): the 16-lane groups of
// the ds_read_b128 fragment reads cover the 64 banks once (asserted below per width).  LDS reads
// of the ring are untracked inline asm (a compiler-visible ds_read behind a pending LDS-DMA gets
// a vmcnt(0) that drains the ring); the DMA waits are counted per wave.
//
// C = 256 (Swin-B stage 1, hidden 1024): the register plan above does not fit (x 64 registers,
// y^T 128: that instantiation spills 32-48 VGPRs), so the width has a kernel of its own below,
// mlp_s1_kernel_pc: the two waves of a SIMD share one 32-token tile as an fc1 + GELU producer and
// an fc2 consumer, GELU(H) handed over through LDS.
#include "common.h"
#include "mfma_frag.h"

namespace {

// MSU_EXP: ablation / variant bits for timing experiments only (tools/build_exp.sh); 0 in every
// real build.  2: fragment reads one MFMA ahead instead of three; 4: waves 4-7 staggered by half a
// chunk (measured slower: 169 vs 160 us, r06h); 8: no GELU (identity); 16: no H stores; 32: no fc2
// MFMAs; 64: no fc1 MFMAs (results wrong by design for 8 / 16 / 32 / 64)
#ifndef MSU_EXP
#define MSU_EXP 0
#endif

constexpr int SW = 8, STT = 32 * SW;
constexpr int UH = 32;                      // hidden units per chunk (one barrier per chunk)
constexpr int FD = (MSU_EXP & 2) ? 1 : 3;   // fragment reads in flight ahead of the MFMA using one
constexpr bool STAG = (MSU_EXP & 4) != 0;   // waves 4-7 run half a chunk behind waves 0-3

// The widths the kernel is built for: x, y [M][C], hidden 4 C.  Everything that depends on the
// width is derived here: a slot holds the chunk's W1 rows [32][C] and W2 columns [C][32]
// (128 C bytes: 16 KB at C = 128, 24 KB at 192, 32 KB at 256), both halves C / 16 1-KB DMA
// instructions.  C = 256 shares the slot image, the ring and the DMA; its kernel is
// mlp_s1_kernel_pc below.
template <int C>
struct S1W {
  static_assert(C == 128 || C == 192 || C == 256, "widths with a register plan and a conflict-free slot image");
  static constexpr int SC = C, SH = 4 * C;
  static constexpr int NU = SH / UH;          // chunks per token tile (16 / 24)
  static constexpr int K1 = C / 16;           // fc1 k steps: a lane's 16-B x loads and y stores per tile
  static constexpr int NCT = C / 32;          // 32-channel output tiles of fc2
  static constexpr int CPR = C / 8;           // 16-B columns of a W1 slot row
  // ring slots (147 KB / 128 KB).  C = 128: 6 / 7 / 8 / 9 slots measured 356 / 352-356 / 349-352 /
  // 356-359 us with H stored and 282-286 us without for all four (r07a, run-to-run spread ~3 us);
  // 8 keeps the same 96 KB in flight as the C = 192 ring.  C = 256 (mlp_s1_kernel_pc): 4 slots of
  // 32 KB, what fits beside the GELU(H) hand-over buffers
  static constexpr int NS = C == 192 ? 6 : C == 256 ? 4 : 8;
  static constexpr int W1S = UH * C;          // elements of a slot's W1 image [32][C]
  static constexpr int W2S = C * UH;          // elements of a slot's W2 image [C][32]
  static constexpr int SLOT = W1S + W2S;
  static constexpr int DMA_W1 = W1S * 2 / 1024;         // 1-KB DMA instructions of the W1 image
  static constexpr int DMA_PER_UNIT = SLOT * 2 / 1024;  // ... of a chunk (16 / 24)
  static constexpr int DMA_PER_WAVE = DMA_PER_UNIT / SW;
  static_assert(DMA_PER_WAVE * SW == DMA_PER_UNIT, "whole DMA instructions per wave");
  static_assert(NS >= 4 && (NS - 3) * DMA_PER_WAVE + 2 * (NS - 2) <= 63, "steady-state vmcnt fits the counter");
};

template <int C>
struct S1Lds {
  bf16_t ring[S1W<C>::NS * S1W<C>::SLOT];
  float b1[S1W<C>::SH];
  float b2[C];
};
static_assert(sizeof(S1Lds<128>) <= 160 * 1024 && sizeof(S1Lds<192>) <= 160 * 1024, "LDS");

struct S1Args {
  const bf16_t* x;
  const bf16_t* w1;  // [4 C][C]
  const float* b1;
  const bf16_t* w2;  // [C][4 C]
  const float* b2;
  bf16_t* y;
  bf16_t* hout;      // H_OUT: [M][4 C]
  long M;
};

// index maps: used by the kernel and by the compile-time checks of the slot image
#define S1_MAP __host__ __device__ __forceinline__ constexpr
// hidden unit (within a chunk) held by slot row rho: bits 2 and 3 swapped
S1_MAP int s1_pi(int rho) { return (rho & ~12) | ((rho & 4) << 1) | ((rho & 8) >> 1); }
// 16-B chunk swizzle of a W2 slot row (4 chunks per row)
S1_MAP int w2_swz(int row) { return (row >> 2) & 3; }
// 16-B column swizzle of W1 slot row rho.  C = 192: 384-B rows start on alternating halves of
// the 256-B bank span, so two rows share a value.  C = 128: rows are one whole bank span, every
// row starts on bank 0, and 16 rows need 16 different values; C = 256: two whole bank spans per
// row, the same (the swizzle stays inside a row's first or second 256 B).
template <int C>
S1_MAP int w1_swz(int rho) { return C == 192 ? (rho >> 1) & 7 : rho & 15; }

// ---- the slot image (byte offsets from the slot's start, a multiple of 256 B).  The fragment
// reads and the DMA below are written with these, and the asserts after them check both.
// 16-B column c of W1 slot row rho = w1_row_off(rho) + w1_col_off(c, w1_swz(rho))
template <int C>
S1_MAP uint32_t w1_row_off(int rho) { return (uint32_t)(rho * C * 2); }
S1_MAP uint32_t w1_col_off(int c, int sw) { return 16u * (uint32_t)(c ^ sw); }
// 16-B column c (0 .. 3) of W2 slot row `row` (0 .. C - 1) = w2_row_off(row) + w2_col_off(c, w2_swz(row))
template <int C>
S1_MAP uint32_t w2_row_off(int row) { return (uint32_t)(S1W<C>::W1S * 2 + row * UH * 2); }
S1_MAP uint32_t w2_col_off(int c, int sw) { return 16u * (uint32_t)(c ^ sw); }
// DMA: the W1 image's 16-B piece p (slot row p / CPR) takes this column of its weight row ...
template <int C>
S1_MAP int w1_dma_col(int p) { return (p % S1W<C>::CPR) ^ w1_swz<C>(p / S1W<C>::CPR); }
// ... and the W2 image's piece p (slot row p / 4) this 16-B column of the chunk's 32 hidden units
S1_MAP int w2_dma_col(int p) { return (p & 3) ^ w2_swz(p >> 2); }

// ds_read_b128 resolves bank conflicts within four groups of 16 lanes: lanes {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same plus 32.  Lane i (0 .. 15) of group g (0 .. 3):
constexpr int b128_group_lane(int g, int i) {
  const int l = (g & 1) == 0 ? (i < 4 ? i : i < 8 ? i + 8 : i + 12) : (i < 8 ? i + 4 : i < 12 ? i + 8 : i + 16);
  return l + 32 * (g >> 1);
}
// every fc1 / fc2 fragment read puts each group's 16 lanes on 16 distinct 16-B bank columns
template <int C>
constexpr bool s1_reads_conflict_free() {
  for (int g = 0; g < 4; ++g) {
    for (int ks = 0; ks < S1W<C>::K1; ++ks) {
      unsigned cols = 0;
      for (int i = 0; i < 16; ++i) {
        const int lane = b128_group_lane(g, i), tl = lane & 31, hh = lane >> 5;
        cols |= 1u << (((w1_row_off<C>(tl) + w1_col_off(2 * ks + hh, w1_swz<C>(tl))) >> 4) & 15);
      }
      if (cols != 0xffffu) return false;
    }
    for (int ct = 0; ct < S1W<C>::NCT; ++ct)
      for (int s = 0; s < 2; ++s) {
        unsigned cols = 0;
        for (int i = 0; i < 16; ++i) {
          const int lane = b128_group_lane(g, i), tl = lane & 31, hh = lane >> 5;
          cols |= 1u << (((w2_row_off<C>(32 * ct + tl) + w2_col_off(2 * s + hh, w2_swz(32 * ct + tl))) >> 4) & 15);
        }
        if (cols != 0xffffu) return false;
      }
  }
  return true;
}
// the DMA writes the image the reads expect: piece p lands at byte 16 p of its half of the slot
template <int C>
constexpr bool s1_dma_writes_image() {
  for (int p = 0; p < UH * S1W<C>::CPR; ++p) {
    const int rho = p / S1W<C>::CPR;
    if (w1_row_off<C>(rho) + w1_col_off(w1_dma_col<C>(p), w1_swz<C>(rho)) != 16u * (uint32_t)p) return false;
  }
  for (int p = 0; p < C * 4; ++p) {
    const int row = p >> 2;
    if (w2_row_off<C>(row) + w2_col_off(w2_dma_col(p), w2_swz(row)) != (uint32_t)(S1W<C>::W1S * 2) + 16u * (uint32_t)p)
      return false;
  }
  return true;
}
static_assert(s1_reads_conflict_free<128>() && s1_reads_conflict_free<192>() && s1_reads_conflict_free<256>(),
              "slot image: bank conflicts");
static_assert(s1_dma_writes_image<128>() && s1_dma_writes_image<192>() && s1_dma_writes_image<256>(),
              "slot image: DMA and reads disagree");

// s_waitcnt vmcnt(n) for a wave-uniform runtime n (capped: waiting for more is always safe)
MSU_DEV void wait_vmcnt_le(int n) {
  switch (n < 0 ? 0 : (n > 40 ? 40 : n)) {
#define MSU_W(k) case k: wait_vmcnt<k>(); break;
    MSU_W(0) MSU_W(1) MSU_W(2) MSU_W(3) MSU_W(4) MSU_W(5) MSU_W(6) MSU_W(7) MSU_W(8) MSU_W(9)
    MSU_W(10) MSU_W(11) MSU_W(12) MSU_W(13) MSU_W(14) MSU_W(15) MSU_W(16) MSU_W(17) MSU_W(18) MSU_W(19)
    MSU_W(20) MSU_W(21) MSU_W(22) MSU_W(23) MSU_W(24) MSU_W(25) MSU_W(26) MSU_W(27) MSU_W(28) MSU_W(29)
    MSU_W(30) MSU_W(31) MSU_W(32) MSU_W(33) MSU_W(34) MSU_W(35) MSU_W(36) MSU_W(37) MSU_W(38) MSU_W(39)
    MSU_W(40)
#undef MSU_W
    default: wait_vmcnt<0>();
  }
}

template <int OFF>
MSU_DEV bf16x8 ds_b128_untracked(uint32_t addr) {
  bf16x8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}

// chunk q (0 .. NU - 1) of the weights into ring slot `slot`: wave `wave`'s share (C / 64) of the
// chunk's C / 8 1-KB DMA instructions (W1 rows permuted by pi and chunk-swizzled; W2 columns
// chunk-swizzled), every wave of the workgroup alike
template <int C>
MSU_DEV void s1_dma_unit(const S1Args& A, bf16_t* ring, int wave, int lane, int q, int slot) {
  using W = S1W<C>;
  bf16_t* base = ring + slot * W::SLOT;
  const int ln = opaque(lane);
#pragma unroll
  for (int r = 0; r < W::DMA_PER_WAVE; ++r) {
    const int i = wave + SW * r;  // instruction (wave-uniform)
    if (i < W::DMA_W1) {
      const int p = 64 * i + ln, rho = p / W::CPR;
      glds16(A.w1 + (long)(UH * q + s1_pi(rho)) * W::SC + 8 * w1_dma_col<C>(p), base + 512 * i);
    } else {
      const int i2 = i - W::DMA_W1;
      const int p = 64 * i2 + ln, row = p >> 2;
      glds16(A.w2 + (long)row * W::SH + UH * q + 8 * w2_dma_col(p), base + W::W1S + 512 * i2);
    }
  }
}

// Per chunk a wave runs three phases: fc1 (K1 = C / 16 MFMAs), the epilogue (b1, H, GELU: VALU),
// fc2 (2 NCT = C / 16 MFMAs).  In every real build (MSU_EXP = 0) all eight waves run fc1(j),
// epi(j), fc2(j) in the interval after chunk j's barrier.
// The MSU_EXP & 4 variant (STAG; measured slower, r06h) STAGGERS waves 4-7: with one barrier per
// chunk the two waves of a SIMD (w, w + 4) run the phases in phase -- both on MFMAs, then both on
// VALU -- so there waves 4-7 run epi(j - 1), fc2(j - 1), fc1(j) in interval j (their fc1
// accumulator crosses the barrier) and each SIMD pairs one wave's MFMAs with the other's VALU.
// The ring is laid out for that variant too: chunk j - 1's slot may be read up to the end of
// interval j, so the ring prefetches SNS - 2 chunks ahead and interval j refills chunk j - 2's
// slot; one extra interval at the end lets staggered waves finish the last chunk.
template <typename T, bool H_OUT, int C>
__global__ void __launch_bounds__(64 * SW) mlp_s1_kernel(S1Args A) {
  using W = S1W<C>;
  constexpr int SC = W::SC, SH = W::SH, NU = W::NU, SNS = W::NS, K1 = W::K1, NCT = W::NCT;
  constexpr int SLOT = W::SLOT, DMA_PER_WAVE = W::DMA_PER_WAVE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  S1Lds<C>& L = *reinterpret_cast<S1Lds<C>*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, tl = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool late = STAG && wave >= 4;  // wave-uniform
  const long M = A.M;
  const long ntiles = (M + STT - 1) / STT;
  const int G = gridDim.x;
  const long first = blockIdx.x;
  if (first >= ntiles) return;
  const long mine = (ntiles - 1 - first) / G + 1;
  const long nunits = mine * NU;

  for (int s = tid; s < SH; s += 64 * SW) L.b1[s] = A.b1[s];
  for (int s = tid; s < SC; s += 64 * SW) L.b2[s] = A.b2[s];
  __syncthreads();  // before any LDS-DMA is in flight (this barrier drains nothing)

  auto dma_unit = [&](int q, int slot) __attribute__((always_inline)) { s1_dma_unit<C>(A, L.ring, wave, lane, q, slot); };
  // the tile's token rows as fc1's B operand: lane (token tl, half hh) holds k = 16 ks + 8 hh .. + 7
  u32x4 xc[K1];
  auto load_x = [&](long t) __attribute__((always_inline)) {
    const long row = t * STT + 32 * wave + tl;
    const bool ok = row < M;
    const bf16_t* p = A.x + (ok ? row : 0) * SC + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < K1; ++ks) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(p + 16 * ks);
      xc[ks] = ok ? v : u32x4{0u, 0u, 0u, 0u};
    }
  };

  // vector-memory ops this wave issued (wave-uniform), and the count right after each pending
  // chunk's DMA (a queue of SNS - 2: the chunk waited for next first): the vmcnt waits let every
  // younger op stay in flight.  Stores are counted only when the whole wave issues them (full
  // tile rows): an uncounted op only makes a wait stricter.
  int issued = 0;
  int mark[SNS - 2];
  load_x(first);
  issued += K1;
  int mark_x = issued;
#pragma unroll
  for (int s = 0; s < SNS - 2; ++s) {
    if (s < nunits) {
      dma_unit(s % NU, s);
      issued += DMA_PER_WAVE;
    }
    mark[s] = issued;
  }

  f32x16 yacc[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) yacc[ct] = f32x16{0};
  f32x16 h = f32x16{0};  // fc1 accumulator (waves 4-7: carried to the next interval)
  // untracked-read lane addresses (bytes)
  const uint32_t ring0 = lds_u32(L.ring);
  const uint32_t a1_lane = w1_row_off<C>(tl);                    // + slot, + 16 * pos(ks)
  const int w1sw = w1_swz<C>(tl);
  const uint32_t a2_lane = w2_row_off<C>(tl);                    // + slot, + 2048 ct, + 16 * pos
  const int w2sw = w2_swz(tl);                                   // (32 ct + tl: same swizzle)
  const uint32_t b1_lane = lds_u32(L.b1) + 4u * (uint32_t)(8 * hh);
  const uint32_t b2_lane = lds_u32(L.b2) + 4u * (uint32_t)(4 * hh);

  // ---- the three phases of a chunk
  auto fc1 = [&](int slot) __attribute__((always_inline)) {
    const uint32_t a1 = ring0 + (uint32_t)(slot * SLOT * 2) + a1_lane;
    h = f32x16{0};
    bf16x8 wf[FD + 1];
    auto addr1 = [&](int ks) { return a1 + w1_col_off(2 * ks + hh, w1sw); };
    unroll_for<FD>([&](auto KS) { wf[decltype(KS)::value] = ds_b128_untracked<0>(addr1(decltype(KS)::value)); });
    unroll_for<K1>([&](auto KS) {
      constexpr int ks = decltype(KS)::value;
      if constexpr (ks + FD < K1) wf[(ks + FD) % (FD + 1)] = ds_b128_untracked<0>(addr1(ks + FD));
      lds_wait_tie<(ks + FD < K1 ? FD : K1 - 1 - ks)>(wf[ks % (FD + 1)]);
      if constexpr (MSU_EXP & 64) {
        const bf16x8 wv = wf[ks % (FD + 1)];
        const u32x4 xv = xc[ks];
        asm volatile("" ::"v"(wv), "v"(xv));
      } else h = Fmt16<T>::mma32(wf[ks % (FD + 1)], __builtin_bit_cast(bf16x8, xc[ks]), h);
    });
  };
  // + b1, 16-bit H (stored), GELU, 16-bit GELU(H): registers 8s + e <-> hidden 32 q + 16 s + 8 hh + e
  auto epi = [&](int q, long t, u32x4 (&g)[2]) __attribute__((always_inline)) {
    u32x4 bq[4];
    unroll_for<4>([&](auto BI) {
      constexpr int bi = decltype(BI)::value;
      bq[bi] = __builtin_bit_cast(u32x4, ds_b128_untracked<(bi >> 1) * 64 + (bi & 1) * 16>(
                                             b1_lane + 4u * (uint32_t)(UH * q)));
    });
    lds_wait_tie<0>(bq[0], bq[1], bq[2], bq[3]);
    const long hrow = t * STT + 32 * wave + tl;
    const bool hok = hrow < M;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float uu[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        uu[e] = round16<T>(h[8 * s + e] + __uint_as_float(bq[2 * s][e]));
        uu[4 + e] = round16<T>(h[8 * s + 4 + e] + __uint_as_float(bq[2 * s + 1][e]));
      }
      if constexpr (H_OUT) {
        const u32x4 hv = {pack2<T>(uu[0], uu[1]), pack2<T>(uu[2], uu[3]), pack2<T>(uu[4], uu[5]),
                          pack2<T>(uu[6], uu[7])};
        if constexpr (MSU_EXP & 16) {
          const u32x4 hv2 = hv;
          asm volatile("" ::"v"(hv2));
        }
        else if (hok) *reinterpret_cast<u32x4*>(A.hout + hrow * SH + UH * q + 16 * s + 8 * hh) = hv;
      }
      uint32_t gp[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x2 gv = (MSU_EXP & 8) ? f32x2{uu[2 * e], uu[2 * e + 1]}
                                       : gelu_fast2(f32x2{uu[2 * e], uu[2 * e + 1]});  // bitwise two gelu_fast
        gp[e] = pack2<T>(gv.x, gv.y);
      }
      g[s] = u32x4{gp[0], gp[1], gp[2], gp[3]};
    }
    if (H_OUT && !(MSU_EXP & 16) && t * STT + 32 * wave + 32 <= M) issued += 2;
  };
  // y^T[c][t] += W2[c][chunk] . GELU(H)^T: C / 32 32-channel tiles, two 16-deep k steps
  auto fc2 = [&](int slot, const u32x4 (&g)[2]) __attribute__((always_inline)) {
    const uint32_t a2 = ring0 + (uint32_t)(slot * SLOT * 2) + a2_lane;
    auto addr2 = [&](int ct, int s) { return a2 + (uint32_t)(ct * 32 * UH * 2) + w2_col_off(2 * s + hh, w2sw); };
    bf16x8 af[FD + 1];
    unroll_for<FD>([&](auto I) {
      constexpr int i = decltype(I)::value;
      af[i] = ds_b128_untracked<0>(addr2(i % NCT, i / NCT));
    });
    unroll_for<2 * NCT>([&](auto I) {
      constexpr int i = decltype(I)::value, s = i / NCT, ct = i % NCT;
      if constexpr (i + FD < 2 * NCT) af[(i + FD) % (FD + 1)] = ds_b128_untracked<0>(addr2((i + FD) % NCT, (i + FD) / NCT));
      lds_wait_tie<(i + FD < 2 * NCT ? FD : 2 * NCT - 1 - i)>(af[i % (FD + 1)]);
      if constexpr (MSU_EXP & 32) {
        const bf16x8 av = af[i % (FD + 1)];
        const u32x4 gv = g[s];
        asm volatile("" ::"v"(av), "v"(gv));
      } else yacc[ct] = Fmt16<T>::mma32(af[i % (FD + 1)], __builtin_bit_cast(bf16x8, g[s]), yacc[ct]);
    });
  };
  // tile epilogue: y = y^T + b2; lane (token tl) holds channels 32 ct + 8 r4 + 4 hh + i in
  // register 4 r4 + i; a permlane32 swap pairs the halves into 8 consecutive channels per lane
  auto y_out = [&](long t) __attribute__((always_inline)) {
    const long row = t * STT + 32 * wave + tl;
    const bool ok = row < M;
    bf16_t* yr = A.y + (ok ? row : 0) * SC;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      uint32_t w[8];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        u32x4 bq;
        asm volatile("ds_read_b128 %0, %1" : "=v"(bq) : "v"(b2_lane + 4u * (uint32_t)(ct * 32 + 8 * r4)));
        lds_wait_tie<0>(bq);
        w[2 * r4] = pack2<T>(yacc[ct][4 * r4] + __uint_as_float(bq[0]), yacc[ct][4 * r4 + 1] + __uint_as_float(bq[1]));
        w[2 * r4 + 1] = pack2<T>(yacc[ct][4 * r4 + 2] + __uint_as_float(bq[2]),
                                 yacc[ct][4 * r4 + 3] + __uint_as_float(bq[3]));
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const auto s0 = __builtin_amdgcn_permlane32_swap(w[4 * p], w[4 * p + 2], false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(w[4 * p + 1], w[4 * p + 3], false, false);
        const u32x4 v = {s0[0], s1[0], s0[1], s1[1]};
        if (ok) *reinterpret_cast<u32x4*>(yr + ct * 32 + 16 * p + 8 * hh) = v;
      }
      yacc[ct] = f32x16{0};
    }
    if (t * STT + 32 * wave + 32 <= M) issued += 2 * NCT;
  };
  // fc1 of chunk (q, slot) of tile t, after which the last chunk of a tile loads the next tile's x
  auto fc1_step = [&](int q, int slot, long t) __attribute__((always_inline)) {
    if (q == 0) wait_vmcnt_le(issued - mark_x);  // the tile's x rows
    fc1(slot);
    if (q == NU - 1 && t + G < ntiles) {  // xc is free once the tile's last fc1 has issued
      load_x(t + G);
      issued += K1;
      mark_x = issued;
    }
  };

  // interval j (0 .. nunits): chunk j = weights chunk q in ring slot `slot` of tile `tile`;
  // (qp, slotp, tilep) the previous chunk; the DMA issued in interval j is chunk j + SNS - 2
  int q = 0, slot = 0, qn = (SNS - 2) % NU, sn = SNS - 2, qp = 0, slotp = 0;
  long tile = first, tilep = first;
  for (long j = 0; j <= nunits; ++j) {
    const bool cur = j < nunits;
    if (cur) {
      // steady state (full tiles, no tile boundary among the younger ops): a constant count
      constexpr int STEADY = (SNS - 3) * DMA_PER_WAVE + (H_OUT && !(MSU_EXP & 16) ? 2 * (SNS - 2) : 0);
      const int younger = issued - mark[0];
      if (younger >= STEADY) wait_vmcnt<STEADY>();
      else wait_vmcnt_le(younger);
    }
    // chunk j's DMA (every wave's share) has landed; every wave is done with chunk j - 2's slot
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int s = 0; s < SNS - 3; ++s) mark[s] = mark[s + 1];
    if (j + SNS - 2 < nunits) {
      dma_unit(qn, sn);
      issued += DMA_PER_WAVE;
    }
    mark[SNS - 3] = issued;
    qn = qn + 1 == NU ? 0 : qn + 1;
    sn = sn + 1 == SNS ? 0 : sn + 1;
    // one straight sequence for both wave groups (two branch-separated copies of the phases
    // made the register allocator keep both copies' operands: 300+ VGPRs of spills)
    const bool second = late ? j > 0 : cur;  // the epi + fc2 of this interval exists
    const int qe = late ? qp : q, se = late ? slotp : slot;
    const long te = late ? tilep : tile;
    if (late && second) {
      u32x4 g[2];
      epi(qe, te, g);
      fc2(se, g);
      if (qe == NU - 1) y_out(te);
    }
    if (cur) fc1_step(q, slot, tile);
    if (!late && second) {
      u32x4 g[2];
      epi(qe, te, g);
      fc2(se, g);
      if (qe == NU - 1) y_out(te);
    }
    qp = q;
    slotp = slot;
    tilep = tile;
    if (q == NU - 1) tile += G;
    q = q + 1 == NU ? 0 : q + 1;
    slot = slot + 1 == SNS ? 0 : slot + 1;
  }
  wait_vmcnt<0>();  // no LDS-DMA outstanding when the workgroup retires
}

// ---------------------------------------------------------------- C = 256: producer / consumer
// The same arithmetic, ring and slot image with the work of a 32-token tile split between the
// two waves of a SIMD (waves p and p + 4, p = 0 .. 3; workgroup tile: 4 pairs, 128 tokens):
//   * the PRODUCER (wave p) holds x (C / 4 = 64 registers) and the fc1 accumulator; per chunk it
//     runs fc1, + b1, the rounding, the H store and GELU, and writes the packed GELU(H) -- fc2's
//     B operand, 2 x 16 B per lane -- into the pair's hand-over buffer;
//   * the CONSUMER (wave p + 4) holds y^T (C / 2 = 128 registers); per chunk it reads those 32 B
//     back into the same lanes, runs fc2 against the chunk's W2 columns, and stores y per tile.
// The older half of the workgroup has the VALU-heavy role.  The hand-over is double-buffered by
// chunk parity and ordered by the ring's one barrier per chunk: in interval j (the code between
// barrier j and barrier j + 1) the producer works on chunk j (slot j's W1 rows, buffer j & 1) and
// the consumer on chunk j - 1 (slot j - 1's W2 columns, buffer (j - 1) & 1):
//   * the producer's ds_writes of chunk j are waited for (lgkmcnt(0), same asm statement) before
//     it arrives at barrier j + 1, which releases the consumer's reads of them;
//   * the consumer's reads of buffer j & 1 (interval j + 1) have returned (lds_wait_tie ahead of
//     the MFMAs that use them) before it arrives at barrier j + 2, behind which the producer
//     overwrites that buffer with chunk j + 2;
//   * chunk j - 1's slot is read up to the end of interval j, so interval j refills chunk j - 2's
//     slot (with chunk j + NS - 2), as in the kernel above.
// BARRIERS: every wave of a workgroup executes 1 + (nunits + 1) of them, nunits = mine * NU from
// blockIdx, gridDim and M alone: the __syncthreads after the bias copy and one per j = 0 ..
// nunits in whichever role loop the wave runs; the only return is ahead of all of them and is
// uniform over the workgroup, and rows past M only mask loads and stores.  By hand, 256 CUs:
// M = 1: one workgroup, mine = 1, 1 + 33 in all 8 waves (pairs 1-3 work on zero rows); M = 129:
// two workgroups with mine = 1, 1 + 33 each; M = 128 * 257 + 5: 258 tiles on 256 workgroups,
// mine = 2 for workgroups 0 and 1 (1 + 65), 1 for the others (1 + 33).
constexpr int PW = 4, PTT = 32 * PW;  // wave pairs per workgroup; tokens per workgroup tile

template <int C>
struct S1PLds {
  bf16_t ring[S1W<C>::NS * S1W<C>::SLOT];
  float b1[S1W<C>::SH];
  float b2[C];
  uint32_t hand[PW][2][2][64 * 4];  // [pair][chunk parity][k step of fc2][lane]: 16 B per lane
};
static_assert(sizeof(S1PLds<256>) <= 160 * 1024, "LDS");

template <typename T, bool H_OUT, int C>
__global__ void __launch_bounds__(64 * SW) mlp_s1_kernel_pc(S1Args A) {
  using W = S1W<C>;
  constexpr int SC = W::SC, SH = W::SH, NU = W::NU, SNS = W::NS, K1 = W::K1, NCT = W::NCT;
  constexpr int SLOT = W::SLOT, DMA_PER_WAVE = W::DMA_PER_WAVE;
  static_assert(SW == 2 * PW, "a producer and a consumer per SIMD");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  S1PLds<C>& L = *reinterpret_cast<S1PLds<C>*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, tl = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pair = wave & (PW - 1);
  const bool producer = wave < PW;  // wave-uniform
  const long M = A.M;
  const long ntiles = (M + PTT - 1) / PTT;
  const int G = gridDim.x;
  const long first = blockIdx.x;
  if (first >= ntiles) return;  // uniform over the workgroup, ahead of every barrier
  const long mine = (ntiles - 1 - first) / G + 1;
  const long nunits = mine * NU;  // both role loops run j = 0 .. nunits: one barrier each

  for (int s = tid; s < SH; s += 64 * SW) L.b1[s] = A.b1[s];
  for (int s = tid; s < SC; s += 64 * SW) L.b2[s] = A.b2[s];
  __syncthreads();  // before any LDS-DMA is in flight (this barrier drains nothing)

  // both roles issue their wave's share (4 of the chunk's 32 DMA instructions)
  auto dma_unit = [&](int q, int slot) __attribute__((always_inline)) { s1_dma_unit<C>(A, L.ring, wave, lane, q, slot); };

  // Each role counts the vector-memory ops of its own wave (wave-uniform): the producer its x
  // loads (K1 per tile), its DMA share and its H stores (2 per chunk), the consumer its DMA share
  // and its y stores (2 NCT per tile).  mark[]: the count right after each pending chunk's DMA
  // (a queue of SNS - 2, the chunk waited for next first).  Stores are counted only when the
  // whole wave issues them (full tile rows): an uncounted op only makes a wait stricter.
  // Outstanding at most K1 + (SNS - 2) DMA_PER_WAVE + 2 (SNS - 1) (producer, across a tile
  // boundary) and 2 NCT + (SNS - 2) DMA_PER_WAVE (consumer):
  static_assert(K1 + (SNS - 2) * DMA_PER_WAVE + 2 * (SNS - 1) <= 63 && 2 * NCT + (SNS - 2) * DMA_PER_WAVE <= 63,
                "vmcnt fits the counter");
  int issued = 0;
  int mark[SNS - 2];
  // ahead of barrier j: this wave's share of chunk j's DMA has landed.  STEADY: the ops younger
  // than it in steady state (the DMA of chunks j + 1 .. j + SNS - 3, the H stores of intervals
  // j - SNS + 2 .. j - 1)
  auto wait_chunk = [&](auto ST) __attribute__((always_inline)) {
    constexpr int STEADY = decltype(ST)::value;
    const int younger = issued - mark[0];
    if (younger >= STEADY) wait_vmcnt<STEADY>();
    else wait_vmcnt_le(younger);
  };
  // behind barrier j: every wave is done with chunk j - 2's slot; chunk j + SNS - 2 goes there
  int qn = (SNS - 2) % NU, sn = SNS - 2;
  auto refill = [&](long j) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < SNS - 3; ++s) mark[s] = mark[s + 1];
    if (j + SNS - 2 < nunits) {
      dma_unit(qn, sn);
      issued += DMA_PER_WAVE;
    }
    mark[SNS - 3] = issued;
    qn = qn + 1 == NU ? 0 : qn + 1;
    sn = sn + 1 == SNS ? 0 : sn + 1;
  };
  auto prologue = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < SNS - 2; ++s) {
      if (s < nunits) {
        dma_unit(s % NU, s);
        issued += DMA_PER_WAVE;
      }
      mark[s] = issued;
    }
  };
  const uint32_t ring0 = lds_u32(L.ring);
  const uint32_t hand_lane = lds_u32(&L.hand[pair][0][0][0]) + 16u * (uint32_t)lane;  // + 2048 parity, + 1024 s

  if (producer) {
    // the tile's token rows as fc1's B operand: lane (token tl, half hh) holds k = 16 ks + 8 hh .. + 7
    u32x4 xc[K1];
    auto load_x = [&](long t) __attribute__((always_inline)) {
      const long row = t * PTT + 32 * pair + tl;
      const bool ok = row < M;
      const bf16_t* p = A.x + (ok ? row : 0) * SC + 8 * hh;
#pragma unroll
      for (int ks = 0; ks < K1; ++ks) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(p + 16 * ks);
        xc[ks] = ok ? v : u32x4{0u, 0u, 0u, 0u};
      }
    };
    load_x(first);
    issued += K1;
    int mark_x = issued;
    prologue();
    const uint32_t a1_lane = w1_row_off<C>(tl);  // + slot, + 16 * pos(ks)
    const int w1sw = w1_swz<C>(tl);
    const uint32_t b1_lane = lds_u32(L.b1) + 4u * (uint32_t)(8 * hh);
    f32x16 h;
    auto fc1 = [&](int slot) __attribute__((always_inline)) {
      const uint32_t a1 = ring0 + (uint32_t)(slot * SLOT * 2) + a1_lane;
      h = f32x16{0};
      bf16x8 wf[FD + 1];
      auto addr1 = [&](int ks) { return a1 + w1_col_off(2 * ks + hh, w1sw); };
      unroll_for<FD>([&](auto KS) { wf[decltype(KS)::value] = ds_b128_untracked<0>(addr1(decltype(KS)::value)); });
      unroll_for<K1>([&](auto KS) {
        constexpr int ks = decltype(KS)::value;
        if constexpr (ks + FD < K1) wf[(ks + FD) % (FD + 1)] = ds_b128_untracked<0>(addr1(ks + FD));
        lds_wait_tie<(ks + FD < K1 ? FD : K1 - 1 - ks)>(wf[ks % (FD + 1)]);
        h = Fmt16<T>::mma32(wf[ks % (FD + 1)], __builtin_bit_cast(bf16x8, xc[ks]), h);
      });
    };
    // + b1, 16-bit H (stored), GELU, 16-bit GELU(H): registers 8s + e <-> hidden 32 q + 16 s + 8 hh + e
    auto epi = [&](int q, long t, u32x4 (&g)[2]) __attribute__((always_inline)) {
      u32x4 bq[4];
      unroll_for<4>([&](auto BI) {
        constexpr int bi = decltype(BI)::value;
        bq[bi] = __builtin_bit_cast(u32x4, ds_b128_untracked<(bi >> 1) * 64 + (bi & 1) * 16>(
                                               b1_lane + 4u * (uint32_t)(UH * q)));
      });
      lds_wait_tie<0>(bq[0], bq[1], bq[2], bq[3]);
      const long hrow = t * PTT + 32 * pair + tl;
      const bool hok = hrow < M;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float uu[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          uu[e] = round16<T>(h[8 * s + e] + __uint_as_float(bq[2 * s][e]));
          uu[4 + e] = round16<T>(h[8 * s + 4 + e] + __uint_as_float(bq[2 * s + 1][e]));
        }
        if constexpr (H_OUT) {
          const u32x4 hv = {pack2<T>(uu[0], uu[1]), pack2<T>(uu[2], uu[3]), pack2<T>(uu[4], uu[5]),
                            pack2<T>(uu[6], uu[7])};
          if (hok) *reinterpret_cast<u32x4*>(A.hout + hrow * SH + UH * q + 16 * s + 8 * hh) = hv;
        }
        uint32_t gp[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const f32x2 gv = gelu_fast2(f32x2{uu[2 * e], uu[2 * e + 1]});  // bitwise two gelu_fast
          gp[e] = pack2<T>(gv.x, gv.y);
        }
        g[s] = u32x4{gp[0], gp[1], gp[2], gp[3]};
      }
      if (H_OUT && t * PTT + 32 * pair + 32 <= M) issued += 2;
    };

    int q = 0, slot = 0;
    long tile = first;
    for (long j = 0; j <= nunits; ++j) {
      const bool cur = j < nunits;
      if (cur) wait_chunk(std::integral_constant<int, (SNS - 3) * DMA_PER_WAVE + (H_OUT ? 2 * (SNS - 2) : 0)>{});
      // chunk j's DMA (every wave's share) has landed; the consumers are done with chunk j - 2's
      // slot and hand-over buffer
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      refill(j);
      if (cur) {
        if (q == 0) wait_vmcnt_le(issued - mark_x);  // the tile's x rows
        fc1(slot);
        if (q == NU - 1 && tile + G < ntiles) {  // xc is free once the tile's last fc1 has issued
          load_x(tile + G);
          issued += K1;
          mark_x = issued;
        }
        u32x4 g[2];
        epi(q, tile, g);
        // the hand-over, complete before this wave arrives at the next barrier
        asm volatile("ds_write_b128 %0, %1\n\tds_write_b128 %0, %2 offset:1024\n\ts_waitcnt lgkmcnt(0)"
                     :: "v"(hand_lane + 2048u * (uint32_t)(j & 1)), "v"(g[0]), "v"(g[1]) : "memory");
        if (q == NU - 1) tile += G;
        q = q + 1 == NU ? 0 : q + 1;
        slot = slot + 1 == SNS ? 0 : slot + 1;
      }
    }
  } else {
    prologue();
    f32x16 yacc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) yacc[ct] = f32x16{0};
    const uint32_t a2_lane = w2_row_off<C>(tl);  // + slot, + 2048 ct, + 16 * pos
    const int w2sw = w2_swz(tl);                 // (32 ct + tl: same swizzle)
    const uint32_t b2_lane = lds_u32(L.b2) + 4u * (uint32_t)(4 * hh);
    // y^T[c][t] += W2[c][chunk] . GELU(H)^T: C / 32 32-channel tiles, two 16-deep k steps; the
    // two hand-over reads go first and are covered by the first fragment's wait
    auto fc2 = [&](int slot, int par) __attribute__((always_inline)) {
      const uint32_t a2 = ring0 + (uint32_t)(slot * SLOT * 2) + a2_lane;
      const uint32_t hb = hand_lane + 2048u * (uint32_t)par;
      auto addr2 = [&](int ct, int s) { return a2 + (uint32_t)(ct * 32 * UH * 2) + w2_col_off(2 * s + hh, w2sw); };
      bf16x8 g[2];
      g[0] = ds_b128_untracked<0>(hb);
      g[1] = ds_b128_untracked<1024>(hb);
      bf16x8 af[FD + 1];
      unroll_for<FD>([&](auto I) {
        constexpr int i = decltype(I)::value;
        af[i] = ds_b128_untracked<0>(addr2(i % NCT, i / NCT));
      });
      unroll_for<2 * NCT>([&](auto I) {
        constexpr int i = decltype(I)::value, s = i / NCT, ct = i % NCT;
        if constexpr (i + FD < 2 * NCT) af[(i + FD) % (FD + 1)] = ds_b128_untracked<0>(addr2((i + FD) % NCT, (i + FD) / NCT));
        if constexpr (i == 0) lds_wait_tie<(FD < 2 * NCT ? FD : 2 * NCT - 1)>(af[0], g[0], g[1]);
        else lds_wait_tie<(i + FD < 2 * NCT ? FD : 2 * NCT - 1 - i)>(af[i % (FD + 1)]);
        yacc[ct] = Fmt16<T>::mma32(af[i % (FD + 1)], g[s], yacc[ct]);
      });
    };
    // tile epilogue: y = y^T + b2; lane (token tl) holds channels 32 ct + 8 r4 + 4 hh + i in
    // register 4 r4 + i; a permlane32 swap pairs the halves into 8 consecutive channels per lane
    auto y_out = [&](long t) __attribute__((always_inline)) {
      const long row = t * PTT + 32 * pair + tl;
      const bool ok = row < M;
      bf16_t* yr = A.y + (ok ? row : 0) * SC;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        uint32_t w[8];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          u32x4 bq;
          asm volatile("ds_read_b128 %0, %1" : "=v"(bq) : "v"(b2_lane + 4u * (uint32_t)(ct * 32 + 8 * r4)));
          lds_wait_tie<0>(bq);
          w[2 * r4] = pack2<T>(yacc[ct][4 * r4] + __uint_as_float(bq[0]), yacc[ct][4 * r4 + 1] + __uint_as_float(bq[1]));
          w[2 * r4 + 1] = pack2<T>(yacc[ct][4 * r4 + 2] + __uint_as_float(bq[2]),
                                   yacc[ct][4 * r4 + 3] + __uint_as_float(bq[3]));
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const auto s0 = __builtin_amdgcn_permlane32_swap(w[4 * p], w[4 * p + 2], false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(w[4 * p + 1], w[4 * p + 3], false, false);
          const u32x4 v = {s0[0], s1[0], s0[1], s1[1]};
          if (ok) *reinterpret_cast<u32x4*>(yr + ct * 32 + 16 * p + 8 * hh) = v;
        }
        yacc[ct] = f32x16{0};
      }
      if (t * PTT + 32 * pair + 32 <= M) issued += 2 * NCT;
    };

    int qp = 0, slotp = 0;  // chunk j - 1: the one this role works on in interval j
    long tilep = first;
    for (long j = 0; j <= nunits; ++j) {
      if (j < nunits) wait_chunk(std::integral_constant<int, (SNS - 3) * DMA_PER_WAVE>{});
      // chunk j's DMA has landed; the producers' hand-over of chunk j - 1 is complete
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      refill(j);
      if (j > 0) {
        fc2(slotp, (int)((j - 1) & 1));
        if (qp == NU - 1) {
          y_out(tilep);
          tilep += G;
        }
        qp = qp + 1 == NU ? 0 : qp + 1;
        slotp = slotp + 1 == SNS ? 0 : slotp + 1;
      }
    }
  }
  wait_vmcnt<0>();  // no LDS-DMA outstanding when the workgroup retires
}

int num_cus_s1() {
  static const int cus = [] {
    int n = 0, dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return n;
  }();
  return cus;
}

// C = 256 takes the producer / consumer kernel (128-token workgroup tiles), the other widths the
// one-role kernel (256-token tiles)
template <typename T, bool H_OUT, int C>
int launch_s1(const S1Args& a, hipStream_t st) {
  constexpr bool PC = C == 256;
  constexpr int TT = PC ? PTT : STT;
  constexpr size_t LDS = PC ? sizeof(S1PLds<C>) : sizeof(S1Lds<C>);
  void (*kern)(S1Args);
  if constexpr (PC) kern = mlp_s1_kernel_pc<T, H_OUT, C>;
  else kern = mlp_s1_kernel<T, H_OUT, C>;
  static bool attr_set = false;  // one per instantiation: each kernel needs its own attribute
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS) != hipSuccess)
      return -4;
    attr_set = true;
  }
  const long ntiles = (a.M + TT - 1) / TT;
  long grid = num_cus_s1();
  if (grid > ntiles) grid = ntiles;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * SW), LDS, st, a);
  return MSU_CHECK_LAUNCH();
}

}  // namespace

// whether the streamed-weight kernel is built for x, y [M][C] (hidden 4 C)
int msu_mlp_s1_width(int C) { return C == 128 || C == 192 || C == 256; }

// the streamed-weight form of msu_mlp_fused_fwd (mlp_fused.hip dispatches here for the widths of
// msu_mlp_s1_width: Swin-B stage 0, C = 128, Swin-T/S stage 1, C = 192, and Swin-B stage 1, C = 256)
int msu_mlp_s1_launch(int dtype, const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                      void* y, void* h, long M, int C, void* stream) {
  S1Args a{};
  a.x = (const bf16_t*)x;
  a.w1 = (const bf16_t*)w1;
  a.b1 = b1;
  a.w2 = (const bf16_t*)w2;
  a.b2 = b2;
  a.y = (bf16_t*)y;
  a.hout = (bf16_t*)h;
  a.M = M;
  hipStream_t st = (hipStream_t)stream;
#define MSU_S1_WIDTH(CC)                                                \
  if (C == CC) {                                                        \
    if (h != nullptr) {                                                 \
      MSU_DISPATCH16(dtype, T, return (launch_s1<T, true, CC>(a, st))); \
    } else {                                                            \
      MSU_DISPATCH16(dtype, T, return (launch_s1<T, false, CC>(a, st)));\
    }                                                                   \
    return -3;                                                          \
  }
  MSU_S1_WIDTH(128)
  MSU_S1_WIDTH(192)
  MSU_S1_WIDTH(256)
#undef MSU_S1_WIDTH
  return -2;
}
