// K1, wave-specialised weight-stationary form -- the split-bf16 FORWARD of the 3x3x3 stride-1 convolutions with 32-256 channels.
//
// Why (profiles/round3_convws.txt): conv_ws.hip keeps a chunk of weights in LDS, but its two symmetric 4-wave groups swap roles step
// by step, so loads, converts, the epilogue and the weight switches run in series with the MFMAs (ablation: 38 us of MFMA work
// plus 16 us loads, 4-9 convert, 5-7 epilogue, 12-18 switches) and the split form was no faster than the tap-table kernel.
// Here the roles are fixed, as in conv16s (conv_bf16.hip):
//   * waves 0-3 ("MFMA waves", one per SIMD) only read LDS, issue MFMAs and run the epilogue.  Wave w owns plane w of a 4x4x16
//     output tile (four 16-voxel rows = four M-tiles) and both 16-channel N-tiles of the workgroup's 32-channel output group;
//   * waves 4-7 ("loader waves") issue every global load (halo of the next item, its prologue parameters, the next weight
//     chunk), apply the fused InstanceNorm + activation prologue, split to bf16 hi / lo and write the halo image of the NEXT item
//     into the other of two LDS buffers while the MFMA waves work on the current one.  Their loads are compiler-tracked and
//     nothing in an MFMA wave ever waits for them; one barrier per item hands a buffer over.
// Work: a persistent workgroup per CU owns one 32-channel output group and a contiguous range of tiles (contiguous per XCD), walked
// in rounds of T tiles, chunk-outer: item = (tile, 16-channel input chunk).  The accumulators of the round's T tiles stay in
// registers across chunks; a chunk of weights (14 tap pairs x 2 N-tiles x hi / lo, 56 KiB) sits in LDS for the T items of a
// (round, chunk) block and is replaced between two barriers (its global loads are issued one item earlier).
// LDS: weights 57,344 B + two halo buffers (hi + lo, 648 voxels x 32 B each) 82,944 B = 140,288 B.
// The loader waves keep one item of halo loads in flight (requested one MFMA item ahead) beside the next weight chunk's registers;
// two items in flight with the weights fetched at the switch measured slower at every shape.
//
// What the product uses: only the 16^3 layers with >= 128 input channels are routed here (see the route below), and those have at
// most one tile per (workgroup, output group) -- wk.slots = tiles -- so they run the T = 2 instantiation with one tile per round:
// every item starts a block and restages the weights (prefetched into the loader waves' registers one item ahead), so nothing is
// weight-stationary there: the gain comes from the wave specialisation alone.  The multi-tile rounds (T = 4, weights resident for T items) run only for larger
// layers, which are faster on the tap-table kernel today and reach this kernel through cwf_debug_wsp(2) (tests).
//
// Results are bit-identical to conv_bf16_kernel (the tap-table kernel): per output element the same MFMA sequence -- chunk
// ascending, tap pair s = 0..13 ascending, hi.hi, hi.lo, lo.hi into one fp32 accumulator that starts at zero -- and the same
// epilogue (v = acc + bias, then + residual; statistics of v).
#include "conv_args.h"
#include <cstdlib>
#include <type_traits>

#define WSP_NT 2                              // output-channel tiles (of 16) per workgroup
#define WSP_NBW 14                            // uint4 of one weight chunk (hi + lo) per loader thread: 57,344 B / 16 / 256

// stat_rows: output rows (of 16 voxels) per fp32 partial of the statistics -- 1 or 4, as in the tap-table launch this one replaces
struct WspWork { int ngroups, slots, tiles, xcd_perm, stat_rows; };

template <int T>
__global__ __launch_bounds__(512) void convwsp_kernel(const ConvArgsB a, const WspWork wk) {
  constexpr int NT = WSP_NT;
  constexpr int B_IMG = 14 * NT * 1024;                    // one chunk of one weight image (hi or lo)
  constexpr int A_IMG = HALO_NVOX * 32;                    // one halo image (hi or lo)
  constexpr int A_BUF = 2 * A_IMG;                         // one halo buffer (hi + lo)
  extern __shared__ float4 lds4[];
  char* lds = reinterpret_cast<char*>(lds4);
  char* const Bh = lds;
  char* const Bl = lds + B_IMG;
  char* const A0 = lds + 2 * B_IMG;
  const ConvGeom& g = a.g;
  const int nch = g.nchunks;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- work: output-channel group and a contiguous range of spatial tiles
  int cgrp, slot;
  {
    const int b = blockIdx.x;
    if (wk.xcd_perm) {
      const int per = gridDim.x >> 3, j = b >> 3;
      cgrp = j % wk.ngroups;
      slot = (b & 7) * (per / wk.ngroups) + j / wk.ngroups;
    } else {
      cgrp = b % wk.ngroups;
      slot = b / wk.ngroups;
    }
  }
  const int t_begin = (int)(((int64_t)slot * wk.tiles) / wk.slots), t_end = (int)(((int64_t)(slot + 1) * wk.tiles) / wk.slots);
  const int ntw = t_end - t_begin;                         // tiles of this workgroup
  const int nt0 = cgrp * NT;
  const int tiles_per_n = g.tiles_d * g.tiles_h * g.tiles_w;

  if (wave < 4) {
    // =============================================================== MFMA waves
    const int wl = wave;
    const int r = lane & 15, kq = lane >> 4;
    const bool second = (kq >> 1) != 0;
    const int a_lane = ((wl * HALO_H) * HALO_W + r) * 32 + (kq & 1) * 16;
    const int b_lane = lane * 16;

    f32x4 acc[T][4][NT];
#pragma unroll
    for (int k = 0; k < T; ++k)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[k][m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // Statistics: the fp32 partial sums are the tap-table kernel's own -- per lane over the 4 voxels of a row (stat_rows = 1) or of
    // the wave's 4 rows, m outer (stat_rows = 4), from zero; then the same two shuffles -- so that only the float64 summation of those
    // partials (here in registers per sample, then one atomic per wave and channel) differs from it.
    float s1[NT], s2[NT];
    double d1[NT], d2[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) { s1[j] = 0.f; s2[j] = 0.f; d1[j] = 0.0; d2[j] = 0.0; }
    int stats_n = -1;
    auto fold = [&]() { fold_stats(s1, s2, d1, d2); };     // (a closure of its own: called directly from epi, hipcc allocates registers differently)
    auto flush_stats = [&]() {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if (kq == 0) {
          const int co = (nt0 + j) * 16 + r;
          atomic_add_f64(a.stats + ((int64_t)stats_n * g.Cout + co) * 2 + 0, d1[j]);
          atomic_add_f64(a.stats + ((int64_t)stats_n * g.Cout + co) * 2 + 1, d2[j]);
        }
        d1[j] = 0.0; d2[j] = 0.0;
      }
    };

    // epilogue of round tile k (the tap-table kernel's interior fast path): v = acc + bias (+ residual), statistics of v
    auto epilogue = [&](int tile, auto KK) {
      constexpr int k = decltype(KK)::value;
      int n, td, th, tw;
      tile_pos(g, tiles_per_n, tile, n, td, th, tw);
      if (a.stats && n != stats_n) {
        if (stats_n >= 0) flush_stats();
        stats_n = n;
      }
      float bvj[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) bvj[j] = a.bias ? a.bias[(nt0 + j) * 16 + r] : 0.f;
      // (this row loop is a copy of conv_bf16.hip's fast-path epilogue, as are conv_ws.hip's and conv_wsd.hip's, and must stay equal to it)
      auto epi = [&](auto HR, auto HT) {
        constexpr bool HAS_RES = decltype(HR)::value, HAS_STATS = decltype(HT)::value;
        unsigned yo[4], ro[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {                      // opaque copies: keep the zero-extension in this block (saddr form)
          yo[i] = epi_lane_off(kq * 4 + i, g.y_ldc, nt0 * 16 + r);
          if (HAS_RES) ro[i] = epi_lane_off(kq * 4 + i, a.r_ldc, nt0 * 16 + r);
        }
        const int od = td * 4 + wl;
        float rv[4][NT][4];
        if (HAS_RES) {                                     // all residual loads first: one latency per tile, not four
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const int64_t vox0 = (((int64_t)n * g.Do + od) * g.Ho + th * 4 + m) * g.Wo + tw * 16;
            const char* rb = reinterpret_cast<const char*>(a.residual + vox0 * a.r_ldc);
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
              for (int i = 0; i < 4; ++i) rv[m][j][i] = *reinterpret_cast<const float*>(rb + ro[i] + j * 64);
          }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int64_t vox0 = (((int64_t)n * g.Do + od) * g.Ho + th * 4 + m) * g.Wo + tw * 16;
          char* yb = reinterpret_cast<char*>(a.y + vox0 * g.y_ldc);
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float v = acc[k][m][j][i] + bvj[j];
              if (HAS_RES) v += rv[m][j][i];
              *reinterpret_cast<float*>(yb + yo[i] + j * 64) = v;
              if (HAS_STATS) stat_sums(v, s1[j], s2[j]);
              acc[k][m][j][i] = 0.f;
            }
          if (HAS_STATS && (wk.stat_rows == 1 || m == 3)) fold();
        }
      };
      using T_ = std::true_type; using F_ = std::false_type;
      if (a.residual) { if (a.stats) epi(T_{}, T_{}); else epi(T_{}, F_{}); }
      else            { if (a.stats) epi(F_{}, T_{}); else epi(F_{}, F_{}); }
    };

    // MFMA phase of one item: 14 tap-pair steps on halo buffer `buf` and the resident weight chunk into the accumulators of tile k
    auto mfma_item = [&](int buf, auto KK) {
      constexpr int k = decltype(KK)::value;
      const char* bh = Bh + b_lane;
      const char* bl = Bl + b_lane;
      const char* ah0 = A0 + buf * A_BUF + a_lane;
      const char* al0 = ah0 + A_IMG;
      // Fragment reads pipelined by hand (as in conv_ws): the hi fragments of step s + 1 are requested before the MFMAs of step s,
      // the lo fragments of step s at its head; per accumulator the order stays hi.hi, hi.lo, lo.hi.
      uint4 fa[2][4], fb[2][NT], fl[4], fbl[NT];
      auto rd_hi = [&](auto S, auto P) {
        constexpr int s = decltype(S)::value, p = decltype(P)::value;
        constexpr int c0 = halo_tap_bytes(2 * s), c1 = halo_tap_bytes(2 * s + 1 < 27 ? 2 * s + 1 : 2 * s);   // padded tap: zero weights
        const int to = second ? c1 : c0;
#pragma unroll
        for (int m = 0; m < 4; ++m) fa[p][m] = *reinterpret_cast<const uint4*>(ah0 + to + m * (HALO_W * 32));
#pragma unroll
        for (int j = 0; j < NT; ++j) fb[p][j] = *reinterpret_cast<const uint4*>(bh + (s * NT + j) * 1024);
      };
      auto rd_lo = [&](auto S) {
        constexpr int s = decltype(S)::value;
        constexpr int c0 = halo_tap_bytes(2 * s), c1 = halo_tap_bytes(2 * s + 1 < 27 ? 2 * s + 1 : 2 * s);
        const int to = second ? c1 : c0;
#pragma unroll
        for (int m = 0; m < 4; ++m) fl[m] = *reinterpret_cast<const uint4*>(al0 + to + m * (HALO_W * 32));
#pragma unroll
        for (int j = 0; j < NT; ++j) fbl[j] = *reinterpret_cast<const uint4*>(bl + (s * NT + j) * 1024);
      };
      auto mm = [&](auto P) {
        constexpr int p = decltype(P)::value;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[k][m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[p][m]), __builtin_bit_cast(bf16x8, fb[p][j]), acc[k][m][j], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[k][m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[p][m]), __builtin_bit_cast(bf16x8, fbl[j]), acc[k][m][j], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[k][m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fl[m]), __builtin_bit_cast(bf16x8, fb[p][j]), acc[k][m][j], 0, 0, 0);
      };
      using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
#define WSP_IC(v) std::integral_constant<int, (v)>{}
#define WSP_STEP2(S0)                                                                                          \
      rd_lo(WSP_IC(S0)); rd_hi(WSP_IC((S0) + 1), I1{}); mm(I0{}); __builtin_amdgcn_sched_barrier(0);            \
      rd_lo(WSP_IC((S0) + 1)); if ((S0) + 2 < 14) rd_hi(WSP_IC((S0) + 2 < 14 ? (S0) + 2 : 13), I0{});           \
      mm(I1{}); __builtin_amdgcn_sched_barrier(0);
      rd_hi(I0{}, I0{});
      WSP_STEP2(0) WSP_STEP2(2) WSP_STEP2(4) WSP_STEP2(6) WSP_STEP2(8) WSP_STEP2(10) WSP_STEP2(12)
#undef WSP_STEP2
#undef WSP_IC
    };

    // item sequence: rounds of up to T tiles; per round chunk-outer; item i uses halo buffer i & 1.  Barriers (the loader waves
    // pass the same ones): H before every item (its halo is in place, and this wave has finished the previous item's reads), and
    // before the first item of a (round, chunk) block after the first, E (every MFMA wave is done with the old weights: the loaders
    // replace them between E and H).
    int i = 0;
    for (int t0 = 0; t0 < ntw; t0 += T) {
      const int nk = min(T, ntw - t0);
      for (int c = 0; c < nch; ++c) {
        auto item = [&](auto KK) {
          constexpr int k = decltype(KK)::value;
          if (k == 0 && i > 0) asm volatile("s_barrier" ::: "memory");     // E
          asm volatile("s_barrier" ::: "memory");                          // H
          mfma_item(i & 1, KK);
          if (c == nch - 1) epilogue(t_begin + t0 + k, KK);
          ++i;
        };
        item(std::integral_constant<int, 0>{});
        if (T > 1 && nk > 1) item(std::integral_constant<int, (T > 1 ? 1 : 0)>{});
        if (T > 2 && nk > 2) item(std::integral_constant<int, (T > 2 ? 2 : 0)>{});
        if (T > 3 && nk > 3) item(std::integral_constant<int, (T > 3 ? 3 : 0)>{});
      }
    }
    if (a.stats && stats_n >= 0) flush_stats();
  } else {
    // =============================================================== loader waves
    const int tg = tid - 256;
    const int ni = ntw * nch;                              // items of this workgroup
    // item i -> (tile, chunk, first item of its block)
    struct Item { int tile, chunk; bool first; };
    auto item_of = [&](int it) {
      const int per_round = T * nch;
      const int rd = it / per_round, w = it - rd * per_round;
      const int nk = min(T, ntw - rd * T);
      const int c = w / nk, k = w - c * nk;
      Item o; o.tile = t_begin + rd * T + k; o.chunk = c; o.first = k == 0;
      return o;
    };

    // ---- weights of one chunk: global -> registers (issued one item ahead) -> LDS between barriers E and H
    u32x4 wpf[WSP_NBW];
    const uint4* wsrc = a.wpk + (int64_t)g.cls_wbase16[0] * 128;
    auto w_issue = [&](int chunk) {
      int tgo = tg;
      asm volatile("" : "+v"(tgo));                        // (opaque: addresses are formed one by one, not hoisted out of the loop)
#pragma unroll
      for (int i = 0; i < WSP_NBW; ++i) {
        const int e = tgo + 256 * i;                        // uint4 index in [image][step][j][lane]
        const int img = e / (14 * NT * 64), e2 = e - img * (14 * NT * 64);
        const int ln = e2 & 63, blk = e2 >> 6;
        const int j = blk % NT, s = blk / NT;
        const uint4* p = wsrc + ((int64_t)(chunk * 14 + s) * g.ntiles + nt0 + j) * 128 + ln * 2 + img;
        wpf[i] = *reinterpret_cast<const u32x4*>(p);
      }
    };
    auto w_write = [&]() {
      int wb = tg * 16;
      asm volatile("" : "+v"(wb));
#pragma unroll
      for (int i = 0; i < WSP_NBW; ++i) *reinterpret_cast<u32x4*>(Bh + wb + i * 4096) = wpf[i];     // (the lo image follows the hi image)
    };

    // ---- halo staging: slot i of this thread holds voxel (tg >> 2) + 64 i, channel quad q = tg & 3
    const int q = tg & 3;
    const int vox0 = tg >> 2;
    const int iw_0 = vox0 % HALO_W, row_0 = vox0 / HALO_W;
    const bool plain = a.in_scale == nullptr && a.in_slope == 1.f;
    f32x4 pf[HALO_SLOTS];
    f32x4 pf_sc, pf_sh;
    unsigned pf_inb = 0u;
    auto issue = [&](int it) {
      const Item itm = item_of(it);
      const int tile = itm.tile, chunk = itm.chunk;
      int n, td, th, tw;
      tile_pos(g, tiles_per_n, tile, n, td, th, tw);
      const int id0 = td * 4 - 1, ih0 = th * 4 - 1, iw0 = tw * 16 - 1;
      const char* xb = reinterpret_cast<const char*>(a.x + (int64_t)n * g.Di * g.Hi * g.Wi * g.x_ldc + chunk * 16);
      const unsigned ldc4 = (unsigned)g.x_ldc * 4u;
      unsigned inb = 0u;
      int iw = iw_0, row = row_0;
      asm volatile("" : "+v"(iw), "+v"(row));              // (opaque: per-slot coordinates are recomputed per item, not kept in hoisted registers)
#pragma unroll
      for (int i = 0; i < HALO_SLOTS; ++i) {
        unsigned boff;
        const bool ok = halo_slot_next(g, id0, ih0, iw0, ldc4, q, iw, row, boff);
        pf[i] = *reinterpret_cast<const f32x4*>(xb + boff);
        inb |= ok ? (1u << i) : 0u;
      }
      pf_inb = inb;
      const float* scp = a.in_scale ? a.in_scale + (int64_t)n * g.Cin + chunk * 16 : a.x;
      const float* shp = a.in_scale ? a.in_shift + (int64_t)n * g.Cin + chunk * 16 : a.x;
      pf_sc = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(scp) + q * 16);
      pf_sh = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(shp) + q * 16);
    };
    auto convert = [&](int buf) {                          // the staged item -> halo buffer buf (item parity)
      const float slope = a.in_slope;
      // activation without a norm (in_scale null, slope != 1): scale 1, shift 0, as the tap-table kernel applies it (the two
      // parameter loads then read a placeholder)
      const bool has_norm = a.in_scale != nullptr;
      const f32x4 sc = has_norm ? pf_sc : (f32x4){1.f, 1.f, 1.f, 1.f}, sh = has_norm ? pf_sh : (f32x4){0.f, 0.f, 0.f, 0.f};
      const unsigned inb = pf_inb;
      int vbase = (tg >> 2) * 32 + q * 8;                  // byte offset of slot 0 in the image; slot i adds an immediate
      asm volatile("" : "+v"(vbase));
      char* ah = A0 + buf * A_BUF + vbase;
#pragma unroll
      for (int i = 0; i < HALO_SLOTS; ++i) {
        if (i == HALO_SLOTS - 1 && vox0 + HALO_DV * i >= HALO_NVOX) continue;
        float v0 = pf[i][0], v1 = pf[i][1], v2 = pf[i][2], v3 = pf[i][3];
        if (!plain) {
          v0 = act01(fmaf(v0, sc[0], sh[0]), slope); v1 = act01(fmaf(v1, sc[1], sh[1]), slope);
          v2 = act01(fmaf(v2, sc[2], sh[2]), slope); v3 = act01(fmaf(v3, sc[3], sh[3]), slope);
        }
        uint2 h, l;
        split_bf16(v0, v1, h.x, l.x); split_bf16(v2, v3, h.y, l.y);
        const bool was = (inb >> i) & 1u;                  // zero padding applies AFTER the activation
        h.x = was ? h.x : 0u; h.y = was ? h.y : 0u; l.x = was ? l.x : 0u; l.y = was ? l.y : 0u;
        *reinterpret_cast<uint2*>(ah + i * (HALO_DV * 32)) = h;
        *reinterpret_cast<uint2*>(ah + A_IMG + i * (HALO_DV * 32)) = l;
      }
    };

    __builtin_amdgcn_s_setprio(1);
    if (ni > 0) {
      // prologue: item 0's halo and block 0's weights in place before the first barrier H; item 1 requested
      issue(0);
      w_issue(0);
      convert(0);
      w_write();
      if (ni > 1) issue(1);
    }
    // iteration it (the MFMA waves run item it): convert item it + 1 (requested one iteration ago, one MFMA item of latency cover)
    // into the free buffer, request the next block's weights if item it + 1 starts one, then request item it + 2.  (One register
    // set: a second set of halo registers in flight spilled beside the weight registers.)
    for (int it = 0; it < ni; ++it) {
      if (it > 0 && item_of(it).first) {
        asm volatile("s_barrier" ::: "memory");            // E: the old weights are no longer read
        w_write();
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // H: item it's halo (and weights) handed over
      if (it + 1 < ni) {
        convert((it + 1) & 1);
        const Item nx = item_of(it + 1);
        if (nx.first) w_issue(nx.chunk);
        if (it + 2 < ni) issue(it + 2);
      }
    }
  }
}

namespace {
template <int T>
int launch_wsp(const ConvArgsB& a, const WspWork& wk, int grid, hipStream_t st) {
  const size_t lds = (size_t)2 * 14 * WSP_NT * 1024 + (size_t)2 * 2 * HALO_NVOX * 32;
  CWF_MAX_LDS_ONCE((&convwsp_kernel<T>));
  hipLaunchKernelGGL((convwsp_kernel<T>), dim3(grid), dim3(512), lds, st, a, wk);
  CWF_LAUNCH_CHECK();
  return 0;
}
}  // namespace

// Route (measured per launch, batch 2, against the tap-table kernel; profiles/wsp_ab.txt): 128 -> 128 @16^3 44 us against 48,
// 128 -> 256 @16^3 50 against 70, 256 -> 128 @16^3 77 against 102 -- but 32 -> 32 @64^3 102 against 101 and 64 -> 64 @32^3 56 against
// 52: with only two or four 16-channel chunks per tile the weight switches and the loader waves' halo stream, not the MFMA work, set
// the pace there (not profiled further).  The product therefore routes layers with >= 128 input channels and >= 128 (tile, output
// group) units.
// cwf_debug_wsp: 1 = that route, 0 = never (tests: the tap-table kernel's result), 2 = every eligible layer.  Returns the old value.
static int g_wsp = 1;
extern "C" int cwf_debug_wsp(int v) { const int old = g_wsp; g_wsp = v; return old; }
// tests: launches of this kernel so far (host-side count, so that a test can tell that a launch took this route)
static long long g_wsp_launches = 0;
extern "C" long long cwf_debug_wsp_launches() { return g_wsp_launches; }
static const int g_wsp_min_cin = 128, g_wsp_min_units = 128;

// Returns 1 and launches if the layer is one this kernel takes (split-bf16 3x3x3 stride-1 forward, Cin a multiple of 16 and >= 32,
// Cout a multiple of 32, extents multiples of the 4x4x16 tile, no groups, output scale or norm-backward operands); 0 = the caller
// goes on to the next route.  The launch status is returned through *rc.
int cwf_try_conv_wsp(int op, int x3, int cfg_mt, int cfg_wm, ConvArgsB& a, hipStream_t st, int* rc) {
  const ConvGeom& g = a.g;
  if (!g_wsp || !x3 || cwf_ws_takes_x3()) return 0;
  if (op != CWF_CONV3_S1 || a.groups || a.out_scale || a.nb_x) return 0;
  if (g.Cin < 32 || (g.Cin & 15) || (g.Cout & 31)) return 0;
  if ((g.Do & 3) || (g.Ho & 3) || (g.Wo & 15)) return 0;
  if (g.x_ldc < g.Cin || (g.x_ldc & 3)) return 0;
  if ((int64_t)g.Di * g.Hi * g.Wi * g.x_ldc * 4 >= (1ll << 31)) return 0;      // 32-bit halo offsets within a sample
  // the statistics' fp32 partials can follow the tap-table configurations with one row per wave (MT = 1) or one plane per wave
  // (MT = 4, WM = 4: tile 4x4x16); under any other the layer stays there
  if (a.stats && !(cfg_mt == 1 || (cfg_mt == 4 && cfg_wm == 4))) return 0;
  WspWork wk;
  wk.stat_rows = cfg_mt;
  wk.ngroups = g.Cout / 32;
  if (wk.ngroups > 32) return 0;
  const int64_t tiles = (int64_t)g.N * (g.Do / 4) * (g.Ho / 4) * (g.Wo / 16);
  if (g_wsp == 1 && (g.Cin < g_wsp_min_cin || tiles * wk.ngroups < g_wsp_min_units)) return 0;
  int e = cwf_build_geom(a.g, op, g.N, g.Di, g.Hi, g.Wi, g.Cin, g.x_ldc, g.Do, g.Ho, g.Wo, g.Cout, g.y_ldc, 16);
  if (e) { *rc = e; return 1; }
  wk.tiles = (int)tiles;
  const int per = (32 / wk.ngroups) * wk.ngroups;         // workgroups per XCD, a multiple of the group count
  wk.slots = 8 * (per / wk.ngroups);
  wk.xcd_perm = 1;
  if (wk.slots > wk.tiles) { wk.slots = wk.tiles; wk.xcd_perm = 0; }
  const int grid = wk.slots * wk.ngroups;
  const int per_wg = (wk.tiles + wk.slots - 1) / wk.slots;
  *rc = per_wg > 2 ? launch_wsp<4>(a, wk, grid, st) : launch_wsp<2>(a, wk, grid, st);
  if (*rc == 0) ++g_wsp_launches;
  return 1;
}
