// K1, wave-specialised weight-in-LDS form -- the SINGLE-bf16 launches (the data gradients) of the 3x3x3 stride-1 convolutions with
// 128 / 256 channels at 16^3.
//
// Why: the tap-table kernel (conv_bf16.hip) gives such a launch 512 workgroups of one 2x2x16 tile x 32 output channels, one 16-voxel
// row per wave: every B fragment a wave fetches from L2 feeds two MFMAs, every workgroup streams the whole K extent of its output
// channels (hi | lo cache lines, of which the single-bf16 form uses the hi half), and the launch moves some 226 MB of weight lines
// from L2 for 0.9 MB of weights (derived from the code, not measured).  conv_ws.hip refuses these layers: too few of its
// (4x4x16 tile, 32 channel) units to fill the chip.
// Here the unit is a 4x4x16 output tile x NT 16-channel output tiles (NT = 1: 256 workgroups at 128 output channels and batch 2,
// NT = 2 where that still gives 256 units), and the roles are fixed as in conv_wsp.hip:
//   * waves 0-3 ("MFMA waves", one per SIMD) only read LDS, issue MFMAs and run the epilogue.  Wave w owns plane w of the tile (four
//     16-voxel rows = four M-tiles): a B fragment read from LDS feeds four MFMAs, and it was fetched from L2 once per workgroup;
//   * waves 4-7 ("loader waves") issue every global load: the fp32 halo of the next 16-channel chunk, converted to bf16 while it is
//     staged, and that chunk's packed weights -- the hi 16-byte granule of each lane's (hi | lo) pair only.
// Item = one 16-channel input chunk of the workgroup's tile; item i lives in LDS buffer i & 1 (halo image + weight chunk), which the
// loader waves fill while the MFMA waves work on the other; one barrier per item hands a buffer over.  A workgroup owns one tile, so
// each weight byte it needs is staged exactly once and nothing has to stay resident: Cin = 128 and Cin = 256 run the same code.
// LDS per workgroup: 2 x (648 voxels x 32 B + 14 x NT x 1 KiB) + 1 KiB x NT for the sums = 71,168 B (NT = 1) or 100,864 B (NT = 2).
// Grid: tiles x Cout / (16 NT) workgroups of 512 threads.
//
// Results: per output element the tap-table kernel's MFMA sequence -- chunk ascending, tap pair 0..13 ascending, one fp32 accumulator
// from zero, then + bias, + residual -- so y is bit-identical to it.  The statistics / norm-backward sums are built from the
// tap-table kernel's own fp32 partials (stat_rows, as in conv_wsp.hip); only the order of their float64 summation differs.
#include "conv_args.h"
#include <cstdlib>
#include <type_traits>

// stat_rows: output rows (of 16 voxels) per fp32 partial of the sums -- 1 or 4, as in the tap-table launch this one replaces
struct WsdWork { int ngroups, stat_rows; };

template <int NT>
__global__ __launch_bounds__(512) void convwsd_kernel(const ConvArgsB a, const WsdWork wk) {
  constexpr int A_IMG = HALO_NVOX * 32;                    // the halo image of one chunk (bf16)
  constexpr int B_IMG = 14 * NT * 1024;                    // the hi weights of one chunk: [tap pair][N-tile][lane] 16 B
  constexpr int BUF = A_IMG + B_IMG;
  extern __shared__ float4 lds4[];
  char* lds = reinterpret_cast<char*>(lds4);
  const ConvGeom& g = a.g;
  const int nch = g.nchunks;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- work: one tile and one group of NT output-channel tiles; the groups of a tile are neighbours (they share its halo in L2)
  // XCD-aware order (workgroups are dealt round-robin over the 8 XCDs, each with its own L2): an XCD takes a contiguous range of tiles
  // with all their output groups, so it reads an eighth of the input and not all of it
  int b = blockIdx.x;
  if ((gridDim.x & 7) == 0) b = (b & 7) * (gridDim.x >> 3) + (b >> 3);
  const int cgrp = b % wk.ngroups, tile = b / wk.ngroups;
  const int nt0 = cgrp * NT;
  const int tiles_per_n = g.tiles_d * g.tiles_h * g.tiles_w;
  int n, td, th, tw;
  tile_pos(g, tiles_per_n, tile, n, td, th, tw);

  if (wave < 4) {
    // =============================================================== MFMA waves
    const int wl = wave;
    const int r = lane & 15, kq = lane >> 4;
    const bool second = (kq >> 1) != 0;
    const int a_lane = ((wl * HALO_H) * HALO_W + r) * 32 + (kq & 1) * 16;
    const int b_lane = A_IMG + lane * 16;

    f32x4 acc[4][NT];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // MFMA phase of one item: 14 tap-pair steps on buffer `buf`.  4 NT MFMAs per step do not cover an LDS read (conv16s, single
    // bf16): the fragment reads run two steps ahead, in a ring of three sets.
    auto mfma_item = [&](int buf) {
      const char* ab = lds + buf * BUF + a_lane;
      const char* bb = lds + buf * BUF + b_lane;
      uint4 fa[3][4], fb[3][NT];
      auto rd = [&](auto S) {
        constexpr int s = decltype(S)::value, p = s % 3;
        constexpr int c0 = halo_tap_bytes(2 * s), c1 = halo_tap_bytes(2 * s + 1 < 27 ? 2 * s + 1 : 2 * s);   // padded tap: zero weights
        const int to = second ? c1 : c0;
#pragma unroll
        for (int m = 0; m < 4; ++m) fa[p][m] = *reinterpret_cast<const uint4*>(ab + to + m * (HALO_W * 32));
#pragma unroll
        for (int j = 0; j < NT; ++j) fb[p][j] = *reinterpret_cast<const uint4*>(bb + (s * NT + j) * 1024);
      };
      auto mm = [&](auto S) {
        constexpr int p = decltype(S)::value % 3;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[p][m]), __builtin_bit_cast(bf16x8, fb[p][j]), acc[m][j], 0, 0, 0);
      };
#define WSD_IC(v) std::integral_constant<int, (v)>{}
#define WSD_STEP(S) if ((S) + 2 < 14) rd(WSD_IC((S) + 2 < 14 ? (S) + 2 : 13)); mm(WSD_IC(S)); __builtin_amdgcn_sched_barrier(0);
      rd(WSD_IC(0)); rd(WSD_IC(1));
      WSD_STEP(0) WSD_STEP(1) WSD_STEP(2) WSD_STEP(3) WSD_STEP(4) WSD_STEP(5) WSD_STEP(6)
      WSD_STEP(7) WSD_STEP(8) WSD_STEP(9) WSD_STEP(10) WSD_STEP(11) WSD_STEP(12) WSD_STEP(13)
#undef WSD_STEP
#undef WSD_IC
    };

    // barrier H before every item (the loader waves pass the same ones): its buffer is in place, and this wave has finished the reads
    // of the item before, whose buffer the loaders fill next
    for (int i = 0; i < nch; ++i) {
      asm volatile("s_barrier" ::: "memory");
      mfma_item(i & 1);
    }

    // ---- epilogue (the tap-table kernel's interior fast path): v = acc + bias (+ residual); sums of v, or the norm-backward sums.
    // fp32 partials as the tap-table kernel forms them: per lane over the 4 voxels of a row (stat_rows = 1) or of the wave's 4 rows,
    // m outer (stat_rows = 4), from zero, then the same two shuffles; summed here in float64.
    float s1[NT], s2[NT];
    double d1[NT], d2[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) { s1[j] = 0.f; s2[j] = 0.f; d1[j] = 0.0; d2[j] = 0.0; }
    float bvj[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bvj[j] = a.bias ? a.bias[(nt0 + j) * 16 + r] : 0.f;
    // (this row loop is a copy of conv_bf16.hip's fast-path epilogue, as are conv_ws.hip's and conv_wsp.hip's, and must stay equal to it)
    auto epi = [&](auto HR, auto HT, auto HN) {
      constexpr bool HAS_RES = decltype(HR)::value, HAS_STATS = decltype(HT)::value, HAS_NB = decltype(HN)::value;
      unsigned yo[4], ro[4], xo[4];
      float nsc[NT], nsh[NT];
#pragma unroll
      for (int i = 0; i < 4; ++i) {                        // opaque copies: keep the zero-extension in this block (saddr form)
        yo[i] = epi_lane_off(kq * 4 + i, g.y_ldc, nt0 * 16 + r);
        if (HAS_RES) ro[i] = epi_lane_off(kq * 4 + i, a.r_ldc, nt0 * 16 + r);
        if (HAS_NB) xo[i] = epi_lane_off(kq * 4 + i, a.nb_ldc, nt0 * 16 + r);
      }
      if (HAS_NB) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          nsc[j] = a.nb_scale[(int64_t)n * g.Cout + (nt0 + j) * 16 + r];
          nsh[j] = a.nb_shift[(int64_t)n * g.Cout + (nt0 + j) * 16 + r];
        }
      }
      const int od = td * 4 + wl;
      float rv[4][NT][4], xv[4][NT][4];                    // all operand loads first: one latency per tile, not four
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int64_t vox0 = (((int64_t)n * g.Do + od) * g.Ho + th * 4 + m) * g.Wo + tw * 16;
        if (HAS_RES) {
          const char* rb = reinterpret_cast<const char*>(a.residual + vox0 * a.r_ldc);
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) rv[m][j][i] = *reinterpret_cast<const float*>(rb + ro[i] + j * 64);
        }
        if (HAS_NB) {
          const char* xb = reinterpret_cast<const char*>(a.nb_x + vox0 * a.nb_ldc);
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[m][j][i] = *reinterpret_cast<const float*>(xb + xo[i] + j * 64);
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
            float v = acc[m][j][i] + bvj[j];
            if (HAS_RES) v += rv[m][j][i];
            *reinterpret_cast<float*>(yb + yo[i] + j * 64) = v;
            if (HAS_NB) nb_sums(v, xv[m][j][i], nsc[j], nsh[j], a.nb_slope, s1[j], s2[j]);
            else if (HAS_STATS) stat_sums(v, s1[j], s2[j]);
          }
        if (HAS_STATS && (wk.stat_rows == 1 || m == 3)) fold_stats(s1, s2, d1, d2);
      }
    };
    using T_ = std::true_type; using F_ = std::false_type;
    if (a.nb_x) { if (a.residual) epi(T_{}, T_{}, T_{}); else epi(F_{}, T_{}, T_{}); }
    else if (a.residual) { if (a.stats) epi(T_{}, T_{}, F_{}); else epi(T_{}, F_{}, F_{}); }
    else            { if (a.stats) epi(F_{}, T_{}, F_{}); else epi(F_{}, F_{}, F_{}); }
    // the four waves' sums meet in LDS (behind the two buffers): one atomic pair per channel and workgroup, summed in wave order
    if (a.stats) {
      double* red = reinterpret_cast<double*>(lds + 2 * BUF);
      if (kq == 0) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          red[((wl * NT + j) * 16 + r) * 2 + 0] = d1[j];
          red[((wl * NT + j) * 16 + r) * 2 + 1] = d2[j];
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (tid < NT * 32) {
        const int which = tid & 1, cr = tid >> 1;          // cr = j * 16 + r
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) sum += red[((w * NT) * 16 + cr) * 2 + which];
        atomic_add_f64(a.stats + ((int64_t)n * g.Cout + nt0 * 16 + cr) * 2 + which, sum);
      }
    }
  } else {
    // =============================================================== loader waves
    constexpr int TG = 256, DV = HALO_DV, SLOTS = HALO_SLOTS;      // loader threads and their halo staging slots (conv_args.h)
    constexpr int NBW = (B_IMG / 16 + TG - 1) / TG;        // weight granules per thread: 4 (the last half used) or 7
    const int tg = tid - 256;
    // ---- weights of one chunk, hi granules only: global -> registers (with the halo) -> LDS
    u32x4 wpf[NBW];
    const uint4* wsrc = a.wpk + (int64_t)g.cls_wbase16[0] * 128;
    // ---- halo staging: slot i of this thread holds voxel (tg >> 2) + DV i, channel quad q = tg & 3
    const int q = tg & 3;
    const int vox0 = tg >> 2;
    const int iw_0 = vox0 % HALO_W, row_0 = vox0 / HALO_W;
    const int id0 = td * 4 - 1, ih0 = th * 4 - 1, iw0 = tw * 16 - 1;
    // A workgroup owns ONE tile: which voxel each staging slot reads, whether it lies in the volume, and which weight granules this
    // thread fetches are the same for every chunk, so they are worked out once; a chunk's loads are scalar base + these offsets.
    unsigned xoff[SLOTS], woff[NBW];
    unsigned pf_inb = 0u;
    {
      const unsigned ldc4 = (unsigned)g.x_ldc * 4u;
      int iw = iw_0, row = row_0;
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        // (halo_slot_next of conv_args.h written out, and to stay equal to it: through the helper hipcc orders this block differently)
        const int idd = (row * 43) >> 8, ih = row - idd * HALO_H;            // row / 6 for row < 48
        const int gd = id0 + idd, gh = ih0 + ih, gw = iw0 + iw;
        const bool ok = (row < HALO_D * HALO_H) & ((unsigned)gd < (unsigned)g.Di) & ((unsigned)gh < (unsigned)g.Hi) & ((unsigned)gw < (unsigned)g.Wi);
        iw += DV % HALO_W; row += DV / HALO_W;             // DV voxels on
        if (iw >= HALO_W) { iw -= HALO_W; ++row; }
        const unsigned lin = (unsigned)((gd * g.Hi + gh) * g.Wi + gw) * ldc4 + (unsigned)q * 16u;
        xoff[i] = ok ? lin : (unsigned)q * 16u;            // (clamped: the load itself is unconditional)
        pf_inb |= ok ? (1u << i) : 0u;
      }
#pragma unroll
      for (int i = 0; i < NBW; ++i) {
        int e = tg + TG * i;                               // granule index in [tap pair][j][lane]
        if (e >= B_IMG / 16) e = 0;                        // (clamped likewise)
        const int ln = e & 63, blk = e >> 6;
        const int j = blk % NT, s = blk / NT;
        woff[i] = (unsigned)((s * g.ntiles + nt0 + j) * 128 + ln * 2) * 16u;
      }
    }
    f32x4 pf[SLOTS];
    const char* xsample = reinterpret_cast<const char*>(a.x + (int64_t)n * g.Di * g.Hi * g.Wi * g.x_ldc);
    auto issue = [&](int chunk) {
      const char* wb = reinterpret_cast<const char*>(wsrc + (int64_t)chunk * 14 * g.ntiles * 128);     // (wave-uniform bases)
      const char* xb = xsample + chunk * 64;
#pragma unroll
      for (int i = 0; i < NBW; ++i) wpf[i] = *reinterpret_cast<const u32x4*>(wb + woff[i]);
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) pf[i] = *reinterpret_cast<const f32x4*>(xb + xoff[i]);
    };
    auto convert = [&](int buf) {                          // the staged chunk -> buffer buf: halo image (zero outside the volume), weights
      const unsigned inb = pf_inb;
      int vbase = buf * BUF + (tg >> 2) * 32 + q * 8;      // byte offset of slot 0; slot i adds an immediate
      asm volatile("" : "+v"(vbase));
      char* ah = lds + vbase;
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        if (DV * (i + 1) > HALO_NVOX && vox0 + DV * i >= HALO_NVOX) continue;
        const bool was = (inb >> i) & 1u;
        uint2 h;
        h.x = was ? pack_bf16(pf[i][0], pf[i][1]) : 0u;
        h.y = was ? pack_bf16(pf[i][2], pf[i][3]) : 0u;
        *reinterpret_cast<uint2*>(ah + i * (DV * 32)) = h;
      }
      int wb = buf * BUF + A_IMG + tg * 16;
      asm volatile("" : "+v"(wb));
#pragma unroll
      for (int i = 0; i < NBW; ++i)
        if (TG * (i + 1) <= B_IMG / 16 || tg + TG * i < B_IMG / 16) *reinterpret_cast<u32x4*>(lds + wb + i * (TG * 16)) = wpf[i];
    };

    __builtin_amdgcn_s_setprio(1);
    // prologue: chunk 0 in place before the first barrier; chunk 1 requested
    issue(0);
    convert(0);
    if (nch > 1) issue(1);
    // iteration it (the MFMA waves run item it): write chunk it + 1 (requested one iteration ago) into the free buffer, request it + 2
    for (int it = 0; it < nch; ++it) {
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // H: item it handed over
      if (it + 1 < nch) {
        convert((it + 1) & 1);
        if (it + 2 < nch) issue(it + 2);
      }
    }
    if (a.stats) asm volatile("s_barrier" ::: "memory");   // (the MFMA waves' reduction of the sums)
  }
}

namespace {
template <int NT>
int launch_wsd(const ConvArgsB& a, const WsdWork& wk, int grid, hipStream_t st) {
  const size_t lds = (size_t)2 * (HALO_NVOX * 32 + 14 * NT * 1024) + 4 * NT * 16 * 2 * sizeof(double);
  CWF_MAX_LDS_ONCE((&convwsd_kernel<NT>));
  hipLaunchKernelGGL((convwsd_kernel<NT>), dim3(grid), dim3(512), lds, st, a, wk);
  CWF_LAUNCH_CHECK();
  return 0;
}
}  // namespace

// Route (measured per launch, batch 2, as launched in the step, against the kernel the launch took before; profiles/wsd_ab.txt):
// 128 -> 128 @16^3 15 us against 31, 256 -> 128 @16^3 24 against 55 (tap-table kernel), 128 -> 256 @16^3 22 against 52 (conv_ws.hip); inside
// the step 25 against 48 -- but 32 -> 32 @64^3 198 against 86 and 64 -> 64 @32^3 46 against 37: with one tile per workgroup nothing is
// reused across tiles, and thousands of workgroups add their sums to a few addresses.  The product therefore routes the small deep
// layers: >= 128 input channels, at most g_wsd_max_tiles 4x4x16 tiles (16^3 at batch 2 has 32) and at least g_wsd_min_units
// (tile, 16 channel) units; larger volumes have the tiles conv_ws.hip's persistent workgroups want.
// cwf_debug_wsd: 1 = that route, 0 = never (tests: the tap-table kernel's result), 2 = every eligible launch, 3 = as 2 with the
// two-tile unit (NT = 2) whatever the unit count (tests).  Returns the old value.
static int g_wsd = 1;
extern "C" int cwf_debug_wsd(int v) { const int old = g_wsd; g_wsd = v; return old; }
// tests: launches of this kernel so far (host-side count)
static long long g_wsd_launches = 0;
extern "C" long long cwf_debug_wsd_launches() { return g_wsd_launches; }
static const int g_wsd_min_cin = 128, g_wsd_min_units = 128, g_wsd_max_tiles = 64;

// Returns 1 and launches if the launch is one this kernel takes (single-bf16 3x3x3 stride 1 from an fp32 input without prologue, Cin
// and Cout multiples of 16, extents multiples of the 4x4x16 tile, no groups, output scale or bf16 images); 0 = the caller goes on to
// the next route.  The launch status is returned through *rc.
int cwf_try_conv_wsd(int op, int x3, int cfg_mt, int cfg_wm, ConvArgsB& a, hipStream_t st, int* rc) {
  const ConvGeom& g = a.g;
  if (!g_wsd || x3) return 0;
  if (op != CWF_CONV3_S1 || a.groups || a.out_scale || a.x16 || a.y16 || a.in_scale || a.in_slope != 1.f) return 0;
  if (g.Cin < 32 || (g.Cin & 15) || (g.Cout & 15)) return 0;
  if (g.Di != g.Do || g.Hi != g.Ho || g.Wi != g.Wo || (g.Do & 3) || (g.Ho & 3) || (g.Wo & 15)) return 0;
  if (g.x_ldc < g.Cin || (g.x_ldc & 3)) return 0;
  if ((int64_t)g.Di * g.Hi * g.Wi * g.x_ldc * 4 >= (1ll << 31)) return 0;      // 32-bit halo offsets within a sample
  // the sums' fp32 partials can follow the tap-table configurations with one row per wave (MT = 1) or one plane per wave (MT = 4,
  // WM = 4: tile 4x4x16); under any other the launch stays there
  if (a.stats && !(cfg_mt == 1 || (cfg_mt == 4 && cfg_wm == 4))) return 0;
  const int64_t tiles = (int64_t)g.N * (g.Do / 4) * (g.Ho / 4) * (g.Wo / 16);
  const int64_t units = tiles * (g.Cout / 16);
  if (units > (1 << 24)) return 0;
  if (g_wsd == 1 && (g.Cin < g_wsd_min_cin || tiles > g_wsd_max_tiles || units < g_wsd_min_units)) return 0;
  // two output tiles per workgroup halve the halo traffic and the LDS reads per MFMA: taken where 256 such units remain
  const bool nt2 = !(g.Cout & 31) && (g_wsd == 3 || units >= 512);
  WsdWork wk;
  wk.stat_rows = cfg_mt;
  wk.ngroups = g.Cout / (nt2 ? 32 : 16);
  int e = cwf_build_geom(a.g, op, g.N, g.Di, g.Hi, g.Wi, g.Cin, g.x_ldc, g.Do, g.Ho, g.Wo, g.Cout, g.y_ldc, 16);
  if (e) { *rc = e; return 1; }
  const int grid = (int)tiles * wk.ngroups;
  *rc = nt2 ? launch_wsd<2>(a, wk, grid, st) : launch_wsd<1>(a, wk, grid, st);
  if (*rc == 0) ++g_wsd_launches;
  return 1;
}
