// K1w (split-bf16 form) -- weight/bias gradient of the conv family on v_mfma_f32_16x16x32_bf16.
//
//   dW[tap][ci][co] = sum_vox xa[vox + tap][ci] * dy[vox][co]     M = ci (16), N = co (16), K = voxels (32 per MFMA)
// Both operands are K-major for this product (the voxel index is the summation index) but live voxel-major in LDS
// ([voxel][16 ch] bf16, written coalesced from NDHWC HBM), so both fragments are fetched with the CDNA4 transposing LDS
// read ds_read_b64_tr_b16: per 16-lane group it takes a 4-voxel x 16-channel block and hands lane i channel i of the
// 4 voxels -- two reads give the 8 consecutive-k bf16 values of a 16x16x32 operand, no shuffles, no second LDS image.
// (EXEC is all ones at every such read: all branches around them are wave-uniform.)
// X3 = true: x = xh + xl, dy = dh + dl -> xh.dh + xh.dl + xl.dh (fp32 accumulate);  X3 = false: xh.dh only.
// Work split, persistent tile walk, partial-slab layout and the reduce step are those of wgrad_mfma.hip.
#include "conv_args.h"
#include <type_traits>
#include <cstdlib>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// Workgroups of the persistent weight-gradient kernels (wgrad16, wgrad_s1, pw_wgrad: 10-16 waves each, most of a CU's registers).
// They run on the side stream BESIDE the main stream's kernels: at one workgroup per CU (256) a main-stream workgroup often finds
// no CU with room and waits for a whole side kernel; fewer workgroups leave CUs to the main stream (an isolated launch is slower,
// the step faster).  Round 2, launches from Python: 192 (99.3 -> 100.1 volumes/s).  Round 3, launch plan (the main stream never
// waits for the host any more): 128 -- 64 / 96 / 128 / 160 / 192 / 256 give 91.3 / 99.9 / 104.8 / 103.7 / 103.1 / 102.6 volumes/s.
// End of round 3 (LDS-DMA weight gradients; only their chain off the main stream): 128 / 160 / 192 / 256 give 110.0 / 110.4 / 110.0 / 108.9: 160.
extern "C" int cwf_wgrad_nsplit(int op, int N, int Do, int Ho, int Wo, int Cin, int Cout);
constexpr int SIDE_WGS = 160;

struct WgArgsB {
  ConvGeom g;
  const float* x; const float* in_scale; const float* in_shift; float in_slope;
  const float* dy; int dy_ldc; float* partial;
  int ngroups, tiles_per_split, total_tiles;
  int64_t slab_floats;
  int cls_slab_base[8];
  // grouped launches (cwf_wgrad with groups: the three sub-regions' head layers): blockIdx.z = group, each with its own
  // x / dy / slab buffer; single-class (3x3x3 stride-1) operators only.  groups == 0: an ordinary launch (blockIdx.z = class)
  int groups;
  const float* x_g[3]; const float* dy_g[3]; float* partial_g[3];
  // wgrad16_kernel only: dy is used as dy * dy_scale[n][co] (the per-(sample, channel) scale of a dropout3d behind the conv, InitConv:
  // Unet_skipconnection.py:29-33 -- its backward is a full-resolution elementwise pass otherwise, the last one before the optimizer)
  const float* dy_scale;
};

// Deliberately the scalar-cast form (two casts and an OR), not pack_bf16 (common.h): the values are the same, but hipcc emits a
// different instruction sequence for it, and swapping the two changes the generated code of every weight-gradient kernel below.
__device__ __forceinline__ unsigned pack_bf16w(float a, float b) {
  const __bf16 x = (__bf16)a, y = (__bf16)b;
  return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
}

// two transposed reads -> one 8-element K fragment.  p0 / p1: this lane's block-row addresses (bf16 element pointers)
__device__ __forceinline__ bf16x8 tr_frag(const unsigned short* p0, const unsigned short* p1) {
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p1));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, v);
}
// the same on LDS byte addresses (the persistent kernels keep per-lane bases in registers and everything else in the ds_read
// immediate): addr = first block row, addr + second = the block row four voxels on
typedef short s16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16x8 tr_frag_at(unsigned addr, unsigned second) {
  const s16x4 u = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)addr);
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(addr + second));
  const s16x8 w = {u[0], u[1], u[2], u[3], v[0], v[1], v[2], v[3]};
  return __builtin_bit_cast(bf16x8, w);
}
// ones operand for the bias row: bf16 1.0 = 0x3F80
__device__ __forceinline__ bf16x8 ones_frag() {
  const s16x8 ones_s = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  return __builtin_bit_cast(bf16x8, ones_s);
}

// tile index -> sample and output origin of a 4 x 4 x 16 tile (tiles_sp = tiles_d * tiles_h * tiles_w)
struct TileOrigin { int n, od0, oh0, ow0; };
__device__ __forceinline__ TileOrigin tile_origin(int tile, int tiles_sp, int tiles_h, int tiles_w) {
  TileOrigin o;
  o.n = tile / tiles_sp; int rem = tile - o.n * tiles_sp;
  const int tile_w = rem % tiles_w; rem /= tiles_w;
  const int tile_h = rem % tiles_h; const int tile_d = rem / tiles_h;
  o.od0 = tile_d * 4; o.oh0 = tile_h * 4; o.ow0 = tile_w * 16;
  return o;
}

// LDS row pitches (in voxels) that make the transposed fragment reads bank-conflict free.  One ds_read_b64_tr_b16 half-wave
// meets two image rows (lane bit kq & 1) x four block rows (bq) x four 8-byte columns (bp); the two image rows must start
// 128 B apart modulo the 256-B bank period.  x image: 32 B per voxel -> pitch = 4 (mod 8) for stride-1 geometries (left
// unpadded for the three stride-2 layers).  dy image, 2*CGW bytes per voxel, 16 voxels per row: CGW = 16 -> pitch 20; CGW = 32:
// the four block rows already span the bank period at a 64-B stride, so every odd row adds a 32-B skew instead (pitch stays 16:
// the layer set with 32 output channels keeps two workgroups per CU, which a wider pitch loses); CGW = 64: left as is.
__host__ __device__ constexpr int wg_x_pitch(int IW, int is) { if (is != 1) return IW; int p = IW; while ((p & 7) != 4) ++p; return p; }
__host__ __device__ constexpr int wg_dy_pitch(int CGW) { return CGW == 16 ? 20 : 16; }
__host__ __device__ constexpr int wg_dy_skew(int CGW) { return CGW == 32 ? 16 : 0; }            // bf16 elements added to odd rows

template <int TPW, int NTW, bool TAPSPLIT, bool X3>
__global__ __launch_bounds__(256) void wgrad_bf16_kernel(const WgArgsB a) {
  constexpr int CG = NTW;
  constexpr int CGW = CG * 16;
  extern __shared__ float4 lds4[];
  const ConvGeom& g = a.g;
  const int nvox_in = g.ID * g.IH * g.IW;
  const int XW = wg_x_pitch(g.IW, g.is), DP = wg_dy_pitch(CGW);   // padded LDS row pitches (voxels)
  const int XIMG = g.ID * g.IH * XW * 16;                          // bf16 elements of one x image
  const int MT = g.TD * g.TH;
  unsigned short* xh = reinterpret_cast<unsigned short*>(lds4);
  unsigned short* xl = xh + XIMG;
  unsigned short* dh = xl + (X3 ? XIMG : 0);
  constexpr int DSK = CGW == 32 ? 16 : 0;
  unsigned short* dl = dh + MT * DP * CGW + (MT / 2 + 1) * DSK;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: wave-dependent choices stay uniform
  const int kq = lane >> 4;
  const int bq = (lane & 15) >> 2, bp = lane & 3;        // transposed-read block row / column quad supplied by this lane
  const int split = blockIdx.x;
  const int chunk = blockIdx.y / a.ngroups, grp = blockIdx.y % a.ngroups;
  const int cls = a.groups ? 0 : blockIdx.z;
  const float* ax_ = a.groups ? a.x_g[blockIdx.z] : a.x;             // (workgroup-uniform: group operands)
  const float* ady_ = a.groups ? a.dy_g[blockIdx.z] : a.dy;
  float* apart_ = a.groups ? a.partial_g[blockIdx.z] : a.partial;
  const int Dc = g.cls_dims[cls][0], Hc = g.cls_dims[cls][1], Wc = g.cls_dims[cls][2];
  const int ntaps = g.cls_ntaps[cls];
  const int* tapofs = g.tapofs + (g.ncls > 1 ? cls * 8 : 0);
  const int co0 = grp * CGW;
  int tapo[TPW];                                         // this wave's tap offsets in the padded image (bf16 elements)
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int t = TAPSPLIT ? wave + 4 * i : i;
    const int o = t < ntaps ? tapofs[t] : 0;
    tapo[i] = ((o / g.IW) * XW + o % g.IW) * 16;
  }

  f32x4 acc[TPW][NTW];
#pragma unroll
  for (int i = 0; i < TPW; ++i)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int tiles_sp = g.tiles_d * g.tiles_h * g.tiles_w;
  const int t_begin = split * a.tiles_per_split;
  const int t_end = min(a.total_tiles, t_begin + a.tiles_per_split);
  const bool vec_dy = (a.dy_ldc & 3) == 0 && (((uintptr_t)ady_) & 15) == 0;
  const int of0 = g.cls_ooff[cls][0], of1 = g.cls_ooff[cls][1], of2 = g.cls_ooff[cls][2];

  // ones operand for the bias row: bf16 1.0 = 0x3F80
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 ones_s = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_s);

  // set-up of the stride-1 fast path (see the K loop)
  const bool geo_s1 = TAPSPLIT && g.is == 1 && g.TD == 4 && g.TH == 4 && g.ID == 6 && g.IH == 6 && g.IW == 18 && ntaps == 27;
  const s16x8 zeros_s = {0, 0, 0, 0, 0, 0, 0, 0};
  const bf16x8 zeros8 = __builtin_bit_cast(bf16x8, zeros_s);
  const bool s1_bias_wave = wave == 3;
  unsigned s1_xa[TPW], s1_da = 0;
  {
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds4;
    const unsigned lane_x = lds_base + (((kq & 1) * 20 + (kq >> 1) * 8 + bq) * 16 + bp * 4) * 2;
    constexpr int DPc = CGW == 16 ? 20 : 16, DSKc = CGW == 32 ? 16 : 0;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const int t = wave + 4 * i;
      s1_xa[i] = lane_x + (t < 27 ? (((t / 9) * 6 + (t / 3) % 3) * 20 + t % 3) * 32 : 0);
    }
    s1_da = lds_base + 36 * 20 * 16 * 2 * (X3 ? 2 : 1) + (((kq & 1) * DPc + (kq >> 1) * 8 + bq) * CGW + (kq & 1) * DSKc + bp * 4) * 2;
  }

  for (int tile = t_begin; tile < t_end; ++tile) {
    const int n = tile / tiles_sp; int rem = tile % tiles_sp;
    const int tile_w = rem % g.tiles_w; rem /= g.tiles_w;
    const int tile_h = rem % g.tiles_h; const int tile_d = rem / g.tiles_h;
    const int od0 = tile_d * g.TD, oh0 = tile_h * g.TH, ow0 = tile_w * 16;
    if (od0 >= Dc || oh0 >= Hc || ow0 >= Wc) continue;
    __syncthreads();
    if (!TAPSPLIT && MT == 16 && g.IW == 16 && g.is == 1) {
      // ---- 1-tap operators (1x1 conv, transposed conv classes): no halo, 256 voxels per tile, almost no MFMA work per
      // byte -- pure streaming.  ALL global loads of the tile (4 x quads + CGW/4 dy quads per thread) are issued before the
      // first conversion, so a tile pays one memory latency instead of one per staging slot (the loop form below measured
      // 1.3 TB/s on the 128^3 layers).
      const int q = tid & 3;
      const int c = chunk * 16 + q * 4;
      const bool cval = c < g.Cin;
      const bool has_norm = a.in_scale != nullptr;
      const bool plain = !has_norm && a.in_slope == 1.f;
      float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
      if (has_norm && cval) {
        sc = *reinterpret_cast<const float4*>(a.in_scale + (int64_t)n * g.Cin + c);
        sh = *reinterpret_cast<const float4*>(a.in_shift + (int64_t)n * g.Cin + c);
      }
      const int id0 = od0 + g.lo[0], ih0 = oh0 + g.lo[1], iw0 = ow0 + g.lo[2];
      constexpr int DSL = CGW / 4;                       // dy quads per thread (16 M-tile rows x 16 voxels x CGW/4 over 256 threads)
      float4 vx[4], vd[DSL];
      unsigned okx = 0, okd = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int v = (tid >> 2) + 64 * i;               // voxel of the 4 x 4 x 16 tile
        const int iw = v & 15, ih = (v >> 4) & 3, idd = v >> 6;
        const int gd = id0 + idd, gh = ih0 + ih, gw = iw0 + iw;
        const bool ok = cval && gd >= 0 && gd < g.Di && gh >= 0 && gh < g.Hi && gw >= 0 && gw < g.Wi;
        const float* px = ax_ + ((((int64_t)n * g.Di + gd) * g.Hi + gh) * g.Wi + gw) * g.x_ldc + c;
        vx[i] = ok ? *reinterpret_cast<const float4*>(px) : make_float4(0.f, 0.f, 0.f, 0.f);
        okx |= ok ? (1u << i) : 0u;
      }
#pragma unroll
      for (int k = 0; k < DSL; ++k) {
        const int e = tid + 256 * k;
        const int vox = e / DSL, cq = e % DSL;
        const int tw = vox & 15, mt = vox >> 4;
        const int od = od0 + (mt >> 2), oh = oh0 + (mt & 3), ow = ow0 + tw;
        const int co = co0 + cq * 4;
        const bool ok = od < Dc && oh < Hc && ow < Wc && co < g.Cout;
        const int64_t gv = (((int64_t)n * g.Do + (od * g.os + of0)) * g.Ho + (oh * g.os + of1)) * g.Wo + (ow * g.os + of2);
        const float* pd = ady_ + gv * a.dy_ldc + co;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) {
          if (vec_dy && co + 3 < g.y_ldc) {
            val = *reinterpret_cast<const float4*>(pd);
            if (co + 1 >= g.Cout) val.y = 0.f;
            if (co + 2 >= g.Cout) val.z = 0.f;
            if (co + 3 >= g.Cout) val.w = 0.f;
          } else {
            val.x = pd[0];
            if (co + 1 < g.Cout) val.y = pd[1];
            if (co + 2 < g.Cout) val.z = pd[2];
            if (co + 3 < g.Cout) val.w = pd[3];
          }
        }
        vd[k] = val;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int v = (tid >> 2) + 64 * i;
        float v0 = vx[i].x, v1 = vx[i].y, v2 = vx[i].z, v3 = vx[i].w;
        if (!plain) {
          v0 = fmaf(v0, sc.x, sh.x); v1 = fmaf(v1, sc.y, sh.y); v2 = fmaf(v2, sc.z, sh.z); v3 = fmaf(v3, sc.w, sh.w);
          v0 = fmaxf(v0, v0 * a.in_slope); v1 = fmaxf(v1, v1 * a.in_slope); v2 = fmaxf(v2, v2 * a.in_slope); v3 = fmaxf(v3, v3 * a.in_slope);
          const bool was = (okx >> i) & 1u;              // zero padding applies after the activation
          v0 = was ? v0 : 0.f; v1 = was ? v1 : 0.f; v2 = was ? v2 : 0.f; v3 = was ? v3 : 0.f;
        }
        uint2 h; h.x = pack_bf16w(v0, v1); h.y = pack_bf16w(v2, v3);
        const int vo = ((v >> 4) * XW + (v & 15)) * 16 + q * 4;
        *reinterpret_cast<uint2*>(xh + vo) = h;
        if (X3) {
          uint2 l;
          l.x = pack_bf16w(v0 - bf16_round(v0), v1 - bf16_round(v1));
          l.y = pack_bf16w(v2 - bf16_round(v2), v3 - bf16_round(v3));
          *reinterpret_cast<uint2*>(xl + vo) = l;
        }
      }
#pragma unroll
      for (int k = 0; k < DSL; ++k) {
        const int e = tid + 256 * k;
        const int vox = e / DSL, cq = e % DSL;
        const int tw = vox & 15, mt = vox >> 4;
        const float4 val = vd[k];
        uint2 h; h.x = pack_bf16w(val.x, val.y); h.y = pack_bf16w(val.z, val.w);
        const int dofs = (mt * DP + tw) * CGW + ((mt + 1) >> 1) * DSK + cq * 4;
        *reinterpret_cast<uint2*>(dh + dofs) = h;
        if (X3) {
          uint2 l;
          l.x = pack_bf16w(val.x - bf16_round(val.x), val.y - bf16_round(val.y));
          l.y = pack_bf16w(val.z - bf16_round(val.z), val.w - bf16_round(val.w));
          *reinterpret_cast<uint2*>(dl + dofs) = l;
        }
      }
      (void)okd;
    } else {
    // ---- x tile (activated) as bf16 hi/lo
    {
      const int q = tid & 3;
      const int c = chunk * 16 + q * 4;
      const bool cval = c < g.Cin;
      const bool has_norm = a.in_scale != nullptr;
      float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
      if (has_norm && cval) {
        sc = *reinterpret_cast<const float4*>(a.in_scale + (int64_t)n * g.Cin + c);
        sh = *reinterpret_cast<const float4*>(a.in_shift + (int64_t)n * g.Cin + c);
      }
      const int id0 = od0 * g.is + g.lo[0], ih0 = oh0 * g.is + g.lo[1], iw0 = ow0 * g.is + g.lo[2];
      for (int v = tid >> 2; v < nvox_in; v += 64) {
        const int iw = v % g.IW; const int t2 = v / g.IW;
        const int ih = t2 % g.IH; const int idd = t2 / g.IH;
        const int gd = id0 + idd, gh = ih0 + ih, gw = iw0 + iw;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cval && gd >= 0 && gd < g.Di && gh >= 0 && gh < g.Hi && gw >= 0 && gw < g.Wi) {
          val = *reinterpret_cast<const float4*>(ax_ + ((((int64_t)n * g.Di + gd) * g.Hi + gh) * g.Wi + gw) * g.x_ldc + c);
          if (has_norm || a.in_slope != 1.f) {
            val.x = cwf_act(val.x * sc.x + sh.x, a.in_slope); val.y = cwf_act(val.y * sc.y + sh.y, a.in_slope);
            val.z = cwf_act(val.z * sc.z + sh.z, a.in_slope); val.w = cwf_act(val.w * sc.w + sh.w, a.in_slope);
          }
        }
        uint2 h; h.x = pack_bf16w(val.x, val.y); h.y = pack_bf16w(val.z, val.w);
        const int vo = (t2 * XW + iw) * 16 + q * 4;
        *reinterpret_cast<uint2*>(xh + vo) = h;
        if (X3) {
          uint2 l;
          l.x = pack_bf16w(val.x - bf16_round(val.x), val.y - bf16_round(val.y));
          l.y = pack_bf16w(val.z - bf16_round(val.z), val.w - bf16_round(val.w));
          *reinterpret_cast<uint2*>(xl + vo) = l;
        }
      }
    }
    // ---- dy tile [MV][CGW] as bf16 hi/lo
    for (int e = tid; e < MT * 16 * (CGW / 4); e += 256) {
      const int vox = e / (CGW / 4), cq = e % (CGW / 4);
      const int tw = vox & 15, mt = vox >> 4;
      const int od = od0 + mt / g.TH, oh = oh0 + mt % g.TH, ow = ow0 + tw;
      const int co = co0 + cq * 4;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (od < Dc && oh < Hc && ow < Wc && co < g.Cout) {
        const int64_t gv = (((int64_t)n * g.Do + (od * g.os + of0)) * g.Ho + (oh * g.os + of1)) * g.Wo + (ow * g.os + of2);
        const float* p = ady_ + gv * a.dy_ldc + co;
        if (vec_dy && co + 3 < g.y_ldc) {
          val = *reinterpret_cast<const float4*>(p);
          if (co + 1 >= g.Cout) val.y = 0.f;
          if (co + 2 >= g.Cout) val.z = 0.f;
          if (co + 3 >= g.Cout) val.w = 0.f;
        } else {
          val.x = p[0];
          if (co + 1 < g.Cout) val.y = p[1];
          if (co + 2 < g.Cout) val.z = p[2];
          if (co + 3 < g.Cout) val.w = p[3];
        }
      }
      uint2 h; h.x = pack_bf16w(val.x, val.y); h.y = pack_bf16w(val.z, val.w);
      const int dofs = (mt * DP + tw) * CGW + ((mt + 1) >> 1) * DSK + cq * 4;   // cumulative skew: rows never overlap
      *reinterpret_cast<uint2*>(dh + dofs) = h;
      if (X3) {
        uint2 l;
        l.x = pack_bf16w(val.x - bf16_round(val.x), val.y - bf16_round(val.y));
        l.y = pack_bf16w(val.z - bf16_round(val.z), val.w - bf16_round(val.w));
        *reinterpret_cast<uint2*>(dl + dofs) = l;
      }
    }
    }
    __syncthreads();

    if (TAPSPLIT && geo_s1) {
      // ---- 3x3x3 stride-1 geometry (6 x 6 x 18 halo, 16 M-tile rows): everything but the per-lane bases is a compile-time
      // immediate, the bias row is folded in by operand selection (ones / zeros), and the transposed reads of tap step f+2
      // are issued before the MFMAs of step f (cf. wgrad16_kernel).  56 tap steps x NTW x 3 MFMAs per tile and wave.
      constexpr int DEPTH = 2;
      constexpr unsigned XLO = 36 * 20 * 16 * 2;                                     // x lo image (bytes past the hi image)
      constexpr unsigned DLO = (16 * (CGW == 16 ? 20 : 16) * CGW + (16 / 2 + 1) * (CGW == 32 ? 16 : 0)) * 2;   // dy lo image
      constexpr int DPc = CGW == 16 ? 20 : 16, DSKc = CGW == 32 ? 16 : 0;
      bf16x8 ah[DEPTH + 1], al[DEPTH + 1], bh[2][NTW], bl[2][NTW];
      auto trf = [&](unsigned addr, unsigned second) {       // two transposed reads -> one 8-element K fragment
        const s16x4 u = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)addr);
        const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(addr + second));
        const s16x8 w = {u[0], u[1], u[2], u[3], v[0], v[1], v[2], v[3]};
        return __builtin_bit_cast(bf16x8, w);
      };
      auto issue = [&](int f) {                              // f = ks * 7 + i, compile-time after unrolling
        const int ks = f / 7, i = f % 7;
        if (i == 0) {
          const unsigned od_ = (2 * ks * DPc * CGW + ks * DSKc) * 2;
#pragma unroll
          for (int j = 0; j < NTW; ++j) {
            bh[ks & 1][j] = trf(s1_da + od_ + j * 32, 4 * CGW * 2);
            if (X3) bl[ks & 1][j] = trf(s1_da + od_ + j * 32 + DLO, 4 * CGW * 2);
          }
        }
        const unsigned ox = (((ks >> 1) * 6 + ((2 * ks) & 3)) * 20) * 32;
        ah[f % (DEPTH + 1)] = trf(s1_xa[i] + ox, 4 * 32);
        if (X3) al[f % (DEPTH + 1)] = trf(s1_xa[i] + ox + XLO, 4 * 32);
      };
#pragma unroll
      for (int f = 0; f < DEPTH; ++f) issue(f);
#pragma unroll
      for (int f = 0; f < 56; ++f) {
        if (f + DEPTH < 56) issue(f + DEPTH);
        __builtin_amdgcn_sched_barrier(0);
        const int ks = f / 7, i = f % 7;
        bf16x8 ahf = ah[f % (DEPTH + 1)], alf = al[f % (DEPTH + 1)];
        if (i == 6) {                                        // wave 3: tap slot 27 = bias row (ones . dy); wave-uniform select
          ahf = s1_bias_wave ? ones : ahf;
          if (X3) alf = s1_bias_wave ? zeros8 : alf;
        }
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahf, bh[ks & 1][j], acc[i][j], 0, 0, 0);
          if (X3) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahf, bl[ks & 1][j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alf, bh[ks & 1][j], acc[i][j], 0, 0, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      continue;
    }
    // ---- K loop: one step = 32 voxels = M-tile rows (2ks, 2ks+1); lane group kq -> row 2ks + (kq&1), voxels 8(kq>>1)..+7
    const int nks = (g.TD * g.TH) >> 1;
#pragma unroll 1
    for (int ks = 0; ks < nks; ++ks) {
      if (!TAPSPLIT && (ks & 3) != wave) continue;           // 1-tap ops: waves split the voxels (wave-uniform)
      const int mt = 2 * ks + (kq & 1);
      const int tw0 = (kq >> 1) * 8 + bq;                    // this lane's block row (first of the two 4-voxel blocks)
      const int vin = ((((mt / g.TH) * g.is) * g.IH + (mt % g.TH) * g.is) * XW + tw0 * g.is) * 16 + bp * 4;
      const int vin4 = vin + 4 * g.is * 16;
      const int vout = (mt * DP + tw0) * CGW + ((mt + 1) >> 1) * DSK + bp * 4;
      const int vout4 = vout + 4 * CGW;
      bf16x8 bh[NTW], bl[NTW];
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        bh[j] = tr_frag(dh + vout + j * 16, dh + vout4 + j * 16);
        if (X3) bl[j] = tr_frag(dl + vout + j * 16, dl + vout4 + j * 16);
      }
#pragma unroll
      for (int i = 0; i < TPW; ++i) {
        const int t = TAPSPLIT ? wave + 4 * i : i;
        if (t > ntaps) continue;                             // wave-uniform
        if (t == ntaps) {                                    // bias row: ones . dy
#pragma unroll
          for (int j = 0; j < NTW; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bh[j], acc[i][j], 0, 0, 0);
            if (X3) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bl[j], acc[i][j], 0, 0, 0);
          }
        } else {
          const int to = tapo[i];
          const bf16x8 ah = tr_frag(xh + vin + to, xh + vin4 + to);
          bf16x8 al;
          if (X3) al = tr_frag(xl + vin + to, xl + vin4 + to);
#pragma unroll
          for (int j = 0; j < NTW; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[j], acc[i][j], 0, 0, 0);
            if (X3) {
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[j], acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[j], acc[i][j], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  float4* out = reinterpret_cast<float4*>(apart_ + (int64_t)(TAPSPLIT ? split : split * 4 + wave) * a.slab_floats);
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int t = TAPSPLIT ? wave + 4 * i : i;
    if (t > ntaps) continue;
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const int64_t blk = (int64_t)a.cls_slab_base[cls] + (((int64_t)chunk * a.ngroups + grp) * (ntaps + 1) + t) * CG + j;
      out[blk * 64 + lane] = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// wgrad_s2: the single-bf16 3x3x3 STRIDE-2 launches of wgrad_bf16_kernel<7, NTW, true, false> (instances TILED_7_1 / TILED_7_2)
// with every global load of a tile in flight at once.  Same grid, tile ranges, LDS images, fragment reads, MFMA order per
// accumulator and slabs as that kernel -- its slabs are bit-equal -- but the geometry is compile-time (2 x 2 x 16 output voxels,
// 5 x 5 x 33 halo, two K-steps; the launcher checks the ConvGeom against it), so
//   * a thread's staging slots are fixed: 825 voxels x 4 channel quads over 256 threads = 13 float4 of x (LDS byte tid * 8 +
//     2048 * slot: the image is unpadded) and NTW float4 of dy; all are loaded, without branches, before the first is converted
//     (a padding slot loads the tensor's first quad and is zeroed at the conversion) -- the loop form paid one memory latency
//     per slot, 15 a tile.  The next tile's loads follow the MFMAs with no barrier between, so they overlap them;
//   * the K loop is straight-line with immediate LDS offsets, the bias row folded in by operand selection (cf. geo_s1);
//   * one LDS buffer and two barriers a tile.  A second buffer (tile t+1's loads issued before tile t's MFMA phase, converted
//     after it, one barrier a tile) measured no faster, alone or in the step (profiles/wgrad_s2_ab.txt), and is not kept.
// dy must be 16-byte aligned with a row pitch that is a multiple of 4 and >= Cout (no scalar dy path; such launches stay on
// wgrad_bf16_kernel).
// ---------------------------------------------------------------------------------------------------
template <int NTW> struct WgS2Lds {
  static constexpr int CGW = NTW * 16;
  static constexpr int NVOX = 5 * 5 * 33, XS = (NVOX * 4 + 255) / 256;     // halo voxels; x staging slots per thread (13)
  static constexpr int DP = wg_dy_pitch(CGW), DSK = wg_dy_skew(CGW);
  static constexpr unsigned XB = NVOX * 16 * 2;                              // x image (bytes), unpadded rows
  static constexpr unsigned DYB = (4 * DP * CGW + 3 * DSK) * 2;              // dy image: 4 rows of 16 voxels, wgrad_bf16_kernel's layout
  static constexpr unsigned BYTES = (XB + DYB + 15) & ~15u;                 // dynamic LDS of a launch
  static constexpr unsigned KSX = 2 * 5 * 33 * 32, KSD = (2 * DP * CGW + DSK) * 2;   // K-step 1 past K-step 0 in the two images
  static_assert(XS == 13 && XB % 16 == 0 && XS * 2048 >= XB, "stride-2 staging slots");
};

template <int NTW>
__global__ __launch_bounds__(256, 2) void wgrad_s2_kernel(const WgArgsB a) {
  typedef WgS2Lds<NTW> L;
  constexpr int CG = NTW, CGW = L::CGW, XS = L::XS, DP = L::DP, DSK = L::DSK;
  extern __shared__ float4 lds4[];
  char* const ldsc = reinterpret_cast<char*>(lds4);
  const ConvGeom& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, bq = (lane & 15) >> 2, bp = lane & 3;
  const int split = blockIdx.x;
  const int chunk = blockIdx.y / a.ngroups, grp = blockIdx.y % a.ngroups;
  const int Dc = g.cls_dims[0][0], Hc = g.cls_dims[0][1], Wc = g.cls_dims[0][2];
  const int co0 = grp * CGW;
  const int of0 = g.cls_ooff[0][0], of1 = g.cls_ooff[0][1], of2 = g.cls_ooff[0][2];

  // per-lane fragment bases (LDS byte addresses): wave w owns taps w, w + 4, ...; slot 27 (wave 3) is the bias row
  const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds4;
  const int tw0 = (kq >> 1) * 8 + bq;
  unsigned xa[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int t = wave + 4 * i;
    xa[i] = lds_base + ((((kq & 1) * 2 * 33 + tw0 * 2) * 16 + bp * 4) * 2) + (t < 27 ? (((t / 9) * 5 + (t / 3) % 3) * 33 + t % 3) * 32 : 0);
  }
  const unsigned da = lds_base + L::XB + ((((kq & 1) * DP + tw0) * CGW + (kq & 1) * DSK + bp * 4) * 2);
  const bool bias_wave = wave == 3;
  const bf16x8 ones = ones_frag();

  f32x4 acc[7][NTW];
#pragma unroll
  for (int i = 0; i < 7; ++i)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int tiles_sp = g.tiles_d * g.tiles_h * g.tiles_w;
  const int t_begin = split * a.tiles_per_split;
  const int t_end = min(a.total_tiles, t_begin + a.tiles_per_split);

  // staging slots of this thread (tile-invariant)
  const int q = tid & 3;
  const int c = chunk * 16 + q * 4;
  const bool cval = c < g.Cin;
  const bool has_norm = a.in_scale != nullptr;
  const bool pro = has_norm || a.in_slope != 1.f;
  const float slope = a.in_slope;

  float4 vx[XS], vd[NTW], sc, sh;
  unsigned okx = 0, okd = 0;

  // every global load of one tile: prologue coefficients, 13 x quads, NTW dy quads; okx / okd: the slots the tiled kernel loads
  // (it writes zero elsewhere)
  auto issue = [&](int tile) {
    const int n = tile / tiles_sp; int rem = tile - n * tiles_sp;
    const int tile_w = rem % g.tiles_w; rem /= g.tiles_w;
    const int tile_h = rem % g.tiles_h; const int tile_d = rem / g.tiles_h;
    const int od0 = tile_d * 2, oh0 = tile_h * 2, ow0 = tile_w * 16;
    sc = make_float4(1.f, 1.f, 1.f, 1.f); sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_norm) {                                        // (a quad past Cin reads quad 0; its slots are zeroed at the conversion)
      sc = *reinterpret_cast<const float4*>(a.in_scale + (int64_t)n * g.Cin + (cval ? c : 0));
      sh = *reinterpret_cast<const float4*>(a.in_shift + (int64_t)n * g.Cin + (cval ? c : 0));
    }
    const int id0 = od0 * 2 + g.lo[0], ih0 = oh0 * 2 + g.lo[1], iw0 = ow0 * 2 + g.lo[2];
    const float* xb = a.x + ((((int64_t)n * g.Di + id0) * g.Hi + ih0) * g.Wi + iw0) * g.x_ldc;    // (uniform; never dereferenced itself)
    okx = 0;
#pragma unroll
    for (int i = 0; i < XS; ++i) {
      const int v = (tid >> 2) + 64 * i;
      const int r = v / 33, iw = v - r * 33, idd = r / 5, ih = r - idd * 5;
      const int gd = id0 + idd, gh = ih0 + ih, gw = iw0 + iw;
      const bool ok = cval & (v < L::NVOX) & ((unsigned)gd < (unsigned)g.Di) & ((unsigned)gh < (unsigned)g.Hi) & ((unsigned)gw < (unsigned)g.Wi);
      const int off = ((idd * g.Hi + ih) * g.Wi + iw) * g.x_ldc + c;
      vx[i] = *reinterpret_cast<const float4*>(ok ? xb + off : a.x);      // (no branch: a padding slot reads the tensor's first quad)
      okx |= ok ? (1u << i) : 0u;
    }
    okd = 0;
#pragma unroll
    for (int k = 0; k < NTW; ++k) {
      const int e = tid + 256 * k;
      const int vox = e / (CGW / 4), cq = e % (CGW / 4);
      const int tw = vox & 15, mt = vox >> 4;
      const int od = od0 + (mt >> 1), oh = oh0 + (mt & 1), ow = ow0 + tw;
      const int co = co0 + cq * 4;
      const bool ok = (od < Dc) & (oh < Hc) & (ow < Wc) & (co < g.Cout);
      const int64_t gv = (((int64_t)n * g.Do + (od * g.os + of0)) * g.Ho + (oh * g.os + of1)) * g.Wo + (ow * g.os + of2);
      vd[k] = *reinterpret_cast<const float4*>(ok ? a.dy + gv * a.dy_ldc + co : a.dy);
      okd |= ok ? (1u << k) : 0u;
    }
  };
  // prologue, rounding and LDS stores of the tile held in vx / vd
  auto convert = [&]() {
#pragma unroll
    for (int i = 0; i < XS; ++i) {
      if ((tid >> 2) + 64 * i >= L::NVOX) continue;
      float4 val = vx[i];
      if (pro) {
        val.x = cwf_act(val.x * sc.x + sh.x, slope); val.y = cwf_act(val.y * sc.y + sh.y, slope);
        val.z = cwf_act(val.z * sc.z + sh.z, slope); val.w = cwf_act(val.w * sc.w + sh.w, slope);
      }
      const bool was = (okx >> i) & 1u;                    // zero padding applies after the activation
      val.x = was ? val.x : 0.f; val.y = was ? val.y : 0.f; val.z = was ? val.z : 0.f; val.w = was ? val.w : 0.f;
      uint2 h; h.x = pack_bf16w(val.x, val.y); h.y = pack_bf16w(val.z, val.w);
      *reinterpret_cast<uint2*>(ldsc + tid * 8 + 2048 * i) = h;
    }
#pragma unroll
    for (int k = 0; k < NTW; ++k) {
      const int e = tid + 256 * k;
      const int vox = e / (CGW / 4), cq = e % (CGW / 4);
      const int tw = vox & 15, mt = vox >> 4;
      const int co = co0 + cq * 4;
      const bool was = (okd >> k) & 1u;
      float4 val = vd[k];
      val.x = was ? val.x : 0.f;
      val.y = was && co + 1 < g.Cout ? val.y : 0.f; val.z = was && co + 2 < g.Cout ? val.z : 0.f; val.w = was && co + 3 < g.Cout ? val.w : 0.f;
      uint2 h; h.x = pack_bf16w(val.x, val.y); h.y = pack_bf16w(val.z, val.w);
      *reinterpret_cast<uint2*>(ldsc + L::XB + ((mt * DP + tw) * CGW + ((mt + 1) >> 1) * DSK + cq * 4) * 2) = h;
    }
  };
  // the tile's two K-steps: all transposed reads, then 14 x NTW MFMAs (K-step order per accumulator as in the tiled kernel)
  auto mfma = [&]() {
    bf16x8 ah[2][7], bh[2][NTW];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int j = 0; j < NTW; ++j) bh[ks][j] = tr_frag_at(da + ks * L::KSD + j * 32, 4 * CGW * 2);
#pragma unroll
      for (int i = 0; i < 7; ++i) ah[ks][i] = tr_frag_at(xa[i] + ks * L::KSX, 4 * 2 * 32);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        const bf16x8 ahf = (i == 6 && bias_wave) ? ones : ah[ks][i];      // wave-uniform select
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahf, bh[ks][j], acc[i][j], 0, 0, 0);
      }
  };

  for (int tile = t_begin; tile < t_end; ++tile) {
    issue(tile);
    __syncthreads();                                       // the previous tile's fragment reads are done
    convert();
    __syncthreads();
    mfma();
  }

  float4* out = reinterpret_cast<float4*>(a.partial + (int64_t)split * a.slab_floats);
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int t = wave + 4 * i;
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const int64_t blk = (int64_t)a.cls_slab_base[0] + (((int64_t)chunk * a.ngroups + grp) * 28 + t) * CG + j;
      out[blk * 64 + lane] = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// wgrad16: weight gradient of the full-resolution 3x3x3 convolutions with <= 16 input and 16 output channels
// (the conv16 layers).  Same producer / consumer structure as conv16_kernel (conv_bf16.hip), for the same measured reasons:
//   * 8-wave persistent workgroups, one per CU, each owning a CONTIGUOUS range of 4x4x16 tiles;
//   * waves 4-7 (loaders) keep two tiles of global loads in flight (x halo 6x6x18 + dy 4x4x16, fp32), apply the recomputed
//     InstanceNorm + activation prologue to x, split both to bf16 hi/lo and fill the other LDS buffer -- straight-line code so
//     that the compiler emits counted vmcnt waits;
//   * waves 0-3 (MFMA) only do transposed LDS reads + MFMAs; wave w owns taps w, w+4, ... (slot 27 = bias row) and keeps its
//     7 accumulators in registers across ALL tiles of the workgroup: no per-tile epilogue at all;
//   * raw s_barrier (lgkmcnt only) hands the buffers over; one slab per workgroup at the end (reduced by cwf_wgrad_reduce).
// ---------------------------------------------------------------------------------------------------
constexpr int W16_DEPTH = 7, WS1_DEPTH = 5;             // LDS-read lookahead of the MFMA waves in tap steps (wgrad16_mfma, wgrad_s1_mfma)
static_assert(WS1_DEPTH < 8 && W16_DEPTH < 8, "the dy fragment of K-step ks+2 reuses the registers of K-step ks");

// x image of the persistent 3x3x3 stride-1 kernels: the 6 x 6 x 18 halo of a 4 x 4 x 16 tile x one 16-channel chunk, voxel-major
// [row][voxel][16 ch] bf16 with rows PADDED to 20 voxels (640 B = 40 granules of 16 B): the two M-tile rows that the lanes of one
// half-wave read in a transposed fragment then start 128 B apart modulo the 256-B bank period, so the ds_read_b64_tr_b16 are
// conflict-free (unpadded: 2-way conflicts, SQ_LDS_BANK_CONFLICT ~ 2k cycles per tile).  The LDS-DMA kernels fill it in pieces of
// 1 KiB (64 lanes x one granule), so there it takes whole pieces.
struct WgXImage {
  static constexpr int XW = 20;                                          // row pitch in voxels (18 + 2 pad)
  static constexpr int XI = 36 * XW * 16;                                // bf16 elements
  static constexpr int XP = (XI * 2 + 1023) / 1024;                      // DMA pieces: 1440 granules -> 23
};
static_assert(WgXImage::XW == wg_x_pitch(18, 1), "x pitch");

// LDS layout of the wgrad16 pair, one definition for kernels and launchers.  A buffer is xh [xl] dh [dl]; the dy image is 4 x 4 rows of
// 16 voxels x 16 channels, padded to 20 voxels like the x image.  DMA = false: two buffers written by converting loader waves
// (wgrad16_kernel<X3>); DMA = true: a four-buffer ring filled by LDS-DMA (wgrad16d_kernel).  Offsets in bytes.
template <bool X3_, bool DMA> struct W16Lds : WgXImage {
  static constexpr bool X3 = X3_;
  static constexpr int DW = 20;                                          // dy row pitch in voxels (16 + 4 pad)
  static constexpr int DI = 16 * DW * 16;                                // bf16 elements of one dy image
  static constexpr int DPC = DI * 2 / 1024;                              // its DMA pieces: 16 rows x 40 granules -> 10
  static constexpr unsigned XLO = DMA ? XP * 1024u : XI * 2u;            // x lo image past the hi image = bytes an x image takes
  static constexpr unsigned DY = XLO * (X3 ? 2 : 1);                     // dy hi image
  static constexpr unsigned DLO = DI * 2u;                               // dy lo image past the hi image
  static constexpr unsigned BUFB = DY + DLO * (X3 ? 2 : 1);              // buffer pitch (DMA: 33,792 B)
  static constexpr int NBUF = DMA ? 4 : 2;
  static constexpr size_t BYTES = (size_t)NBUF * BUFB;                   // dynamic LDS of a launch
  static_assert(DW == wg_dy_pitch(16) && wg_dy_skew(16) == 0 && DI * 2 % 1024 == 0 && BUFB % 16 == 0 && !(X3 && DMA), "wgrad16 layout");
};

#define W16_NVOX HALO_NVOX                              // the x tile of a 4x4x16 dy tile is that tile's halo (conv_args.h)
#define W16_LW 6                                        // loader waves (MFMA waves: 4) -> 640-thread workgroups
#define W16_VPP (W16_LW * 16)                           // voxels staged per pass (4 threads per voxel)
#define W16_XS ((W16_NVOX + W16_VPP - 1) / W16_VPP)     // 7 x staging slots per loader thread
#define W16_DS ((256 + W16_VPP - 1) / W16_VPP)          // 3 dy staging slots per loader thread

// MFMA waves (0-3) of the wgrad16 pair.  L: the pair's LDS layout (operand form, image offsets, buffer pitch and count);
// out: the workgroup's slab.
template <class L>
__device__ __forceinline__ void wgrad16_mfma(unsigned lds_base, int wave, int lane, int niter, float4* out) {
  constexpr bool X3 = L::X3;
  constexpr int XW = L::XW, DW = L::DW;
  const int kq = lane >> 4;
  const int bq = (lane & 15) >> 2, bp = lane & 3;
  f32x4 acc[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const bf16x8 ones = ones_frag();
  // K = 32 voxels per MFMA = M-tile rows (2ks, 2ks+1) x 16 voxels.  Lane group kq reads row 2ks + (kq & 1), voxels
  // 8 (kq >> 1) + [0, 8): the two rows met inside one half-wave are 640 B apart (see the padding note at WgXImage).
  // Addresses are integers (LDS byte addresses): per-tap bases in registers, everything else in the ds_read immediate, so
  // the fully unrolled loop has no address arithmetic (same vector-issue argument as conv16_kernel).
  const unsigned lane_x = lds_base + (((kq & 1) * XW + (kq >> 1) * 8 + bq) * 16 + bp * 4) * 2;
  unsigned xa[7];                                      // x hi image: lane part + tap offset (+ buffer)
  unsigned da = lds_base + L::DY + (((kq & 1) * DW + (kq >> 1) * 8 + bq) * 16 + bp * 4) * 2;   // dy hi image
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int t = wave + 4 * i;
    xa[i] = lane_x + (t < 27 ? (((t / 9) * 6 + (t / 3) % 3) * XW + t % 3) * 32 : 0);
  }
  // Two straight-line copies of the whole tile loop (wave 3's last slot is the bias row).  A tile is 8 K-steps x 7 taps =
  // 56 "tap steps" of 3 MFMAs (48 cycles); the 4 transposed reads of tap step f+2 are issued before the MFMAs of step f
  // (explicit register double-buffering, pinned with sched_barrier: left alone, the compiler issues each read right
  // before its MFMA and every MFMA waits out the LDS latency).
  auto tiles = [&](auto BIAS_) {
    constexpr bool BIAS = decltype(BIAS_)::value;
    // LDS-read lookahead in tap steps.  Split operands: a step is 3 MFMAs = 48 cycles, two steps cover the transposed-read latency.
    // Single-bf16 operands (what the bench runs): ONE MFMA = 16 cycles per step -- at two steps every MFMA waited out most of an
    // LDS round trip (5.6k cycles per tile against 0.9k of MFMAs); seven steps ahead (the most the two-slot dy-fragment ring allows), in registers the lo fragments do not need.
    constexpr int DEPTH = X3 ? 2 : W16_DEPTH;
    for (int it = 0; it < niter; ++it) {
      asm volatile("s_barrier" ::: "memory");          // buffer it & (NBUF - 1) is complete
      bf16x8 ah[DEPTH + 1], al[DEPTH + 1], bh[2], bl[2];
      auto issue = [&](int f) {                        // f = ks * 7 + i, compile-time after unrolling
        const int ks = f / 7, i = f % 7;
        if (i == 0) {
          const unsigned od_ = (2 * ks * DW) * 32;
          bh[ks & 1] = tr_frag_at(da + od_, 4 * 32);
          if (X3) bl[ks & 1] = tr_frag_at(da + od_ + L::DLO, 4 * 32);
        }
        if (!(BIAS && i == 6)) {
          const unsigned ox = (((ks >> 1) * 6 + ((2 * ks) & 3)) * XW) * 32;
          ah[f % (DEPTH + 1)] = tr_frag_at(xa[i] + ox, 4 * 32);
          if (X3) al[f % (DEPTH + 1)] = tr_frag_at(xa[i] + ox + L::XLO, 4 * 32);
        }
      };
#pragma unroll
      for (int f = 0; f < DEPTH; ++f) issue(f);
#pragma unroll
      for (int f = 0; f < 56; ++f) {
        if (f + DEPTH < 56) issue(f + DEPTH);
        __builtin_amdgcn_sched_barrier(0);
        const int ks = f / 7, i = f % 7;
        const bf16x8 bhf = bh[ks & 1];
        if (BIAS && i == 6) {                          // tap slot 27 = bias row (ones . dy)
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bhf, acc[i], 0, 0, 0);
          if (X3) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bl[ks & 1], acc[i], 0, 0, 0);
        } else {
          const bf16x8 ahf = ah[f % (DEPTH + 1)];
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahf, bhf, acc[i], 0, 0, 0);
          if (X3) {
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahf, bl[ks & 1], acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[f % (DEPTH + 1)], bhf, acc[i], 0, 0, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      {                                                // the next buffer of the ring is read next
        constexpr int LAST = L::NBUF - 1;
        const unsigned dlt = ((it & LAST) == LAST) ? (unsigned)(-(int)(LAST * L::BUFB)) : L::BUFB;
#pragma unroll
        for (int i = 0; i < 7; ++i) xa[i] += dlt;
        da += dlt;
      }
    }
  };
  if (wave == 3) tiles(std::true_type{}); else tiles(std::false_type{});
  // one slab per workgroup: [tap slot 0..27][lane][4]   (chunk 0, group 0, CG = 1)
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int t = wave + 4 * i;
    if (t > 27) continue;
    out[(int64_t)t * 64 + lane] = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
  }
}

template <bool X3>
__global__ __launch_bounds__(256 + 64 * W16_LW) void wgrad16_kernel(const WgArgsB a, int total_tiles) {
  using L = W16Lds<X3, false>;
  extern __shared__ float4 lds4[];
  const ConvGeom& g = a.g;
  unsigned short* lds = reinterpret_cast<unsigned short*>(lds4);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the role branch below is provably wave-uniform
  const int tiles_sp = g.tiles_d * g.tiles_h * g.tiles_w;
  // XCD-aware tile map (see conv16_kernel): iteration `it` covers tiles [it*G, (it+1)*G); XCD x takes segment x of it
  const int G = (int)gridDim.x, per = G >> 3;
  const int first = (blockIdx.x & 7) * per + (blockIdx.x >> 3);      // tile(it) = first + it * G
  const int niter = first < total_tiles ? (total_tiles - first + G - 1) / G : 0;   // empty workgroups still write a zero slab

  if (wave < 4) {
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds4;
    wgrad16_mfma<L>(lds_base, wave, lane, niter, reinterpret_cast<float4*>(a.partial + (int64_t)blockIdx.x * a.slab_floats));
  } else {
    // =============================================================== loader waves
    const int lt = tid - 256;
    const int q = lt & 3, c = q * 4;
    const bool cval = c < g.Cin;
    const bool has_norm = a.in_scale != nullptr;
    const float slope = a.in_slope;
    const float sl = (has_norm || slope != 1.f) ? slope : 1.f;
    const int HW = g.Hi * g.Wi;
    int relx[W16_XS], reld[W16_DS];
#pragma unroll
    for (int i = 0; i < W16_XS; ++i) {
      const int v = (lt >> 2) + W16_VPP * i;
      const int iw = v % 18, t2 = v / 18;
      relx[i] = ((t2 / 6) * HW + (t2 % 6) * g.Wi + iw) * g.x_ldc + c;
    }
#pragma unroll
    for (int i = 0; i < W16_DS; ++i) {
      const int v = (lt >> 2) + W16_VPP * i;                  // output voxel: td = v>>6, th = (v>>4)&3, tw = v&15
      reld[i] = (((v >> 6) * g.Ho + ((v >> 4) & 3)) * g.Wo + (v & 15)) * a.dy_ldc + c;
    }
    const bool last_ok = (lt >> 2) + W16_VPP * (W16_XS - 1) < W16_NVOX;
    const bool dlast_ok = (lt >> 2) + W16_VPP * (W16_DS - 1) < 256;
    int xo[W16_XS], dofs[W16_DS];                        // LDS element offsets of this thread's staging slots (padded rows)
#pragma unroll
    for (int i = 0; i < W16_XS; ++i) { const int v = (lt >> 2) + W16_VPP * i; xo[i] = ((v / 18) * L::XW + v % 18) * 16 + q * 4; }
#pragma unroll
    for (int i = 0; i < W16_DS; ++i) { const int v = (lt >> 2) + W16_VPP * i; dofs[i] = ((v >> 4) * L::DW + (v & 15)) * 16 + q * 4; }
    float4 px[1][W16_XS], pd[1][W16_DS];
    unsigned inbx[1] = {0u}, inbd[1] = {0u};
    __builtin_amdgcn_s_setprio(1);
    struct Org { const float* xb; const float* db; bool interior; int id0, ih0, iw0, od0, oh0, ow0, n; };
    auto origin = [&](int tile) {
      Org o;
      const TileOrigin t = tile_origin(tile, tiles_sp, g.tiles_h, g.tiles_w);
      o.n = t.n; o.od0 = t.od0; o.oh0 = t.oh0; o.ow0 = t.ow0;
      o.id0 = o.od0 - 1; o.ih0 = o.oh0 - 1; o.iw0 = o.ow0 - 1;
      o.xb = a.x + ((((int64_t)o.n * g.Di + o.id0) * g.Hi + o.ih0) * g.Wi + o.iw0) * g.x_ldc;
      o.db = a.dy + ((((int64_t)o.n * g.Do + o.od0) * g.Ho + o.oh0) * g.Wo + o.ow0) * a.dy_ldc;
      o.interior = o.id0 >= 0 && o.id0 + 6 <= g.Di && o.ih0 >= 0 && o.ih0 + 6 <= g.Hi && o.iw0 >= 0 && o.iw0 + 18 <= g.Wi &&
                   o.od0 + 4 <= g.Do && o.oh0 + 4 <= g.Ho && o.ow0 + 16 <= g.Wo;
      return o;
    };
    auto issue = [&](const Org& o, auto S) {
      constexpr int SET = decltype(S)::value;
      unsigned mx = 0, md = 0;
      if (o.interior) {
#pragma unroll
        for (int i = 0; i < W16_XS; ++i) {
          const bool ok = cval && (i < W16_XS - 1 || last_ok);
          px[SET][i] = *reinterpret_cast<const float4*>(ok ? o.xb + relx[i] : a.x);
          mx |= ok ? (1u << i) : 0u;
        }
#pragma unroll
        for (int i = 0; i < W16_DS; ++i) {
          const bool ok = i < W16_DS - 1 || dlast_ok;
          pd[SET][i] = *reinterpret_cast<const float4*>(ok ? o.db + reld[i] : a.dy);
          md |= ok ? (1u << i) : 0u;
        }
      } else {
#pragma unroll
        for (int i = 0; i < W16_XS; ++i) {
          const int v = (lt >> 2) + W16_VPP * i;
          const int iw = v % 18, t2 = v / 18;
          const int gd = o.id0 + t2 / 6, gh = o.ih0 + t2 % 6, gw = o.iw0 + iw;
          const bool ok = cval && (i < W16_XS - 1 || last_ok) && (unsigned)gd < (unsigned)g.Di && (unsigned)gh < (unsigned)g.Hi && (unsigned)gw < (unsigned)g.Wi;
          px[SET][i] = *reinterpret_cast<const float4*>(ok ? o.xb + relx[i] : a.x);
          mx |= ok ? (1u << i) : 0u;
        }
#pragma unroll
        for (int i = 0; i < W16_DS; ++i) {
          const int v = (lt >> 2) + W16_VPP * i;
          const bool ok = (i < W16_DS - 1 || dlast_ok) && o.od0 + (v >> 6) < g.Do && o.oh0 + ((v >> 4) & 3) < g.Ho && o.ow0 + (v & 15) < g.Wo;
          pd[SET][i] = *reinterpret_cast<const float4*>(ok ? o.db + reld[i] : a.dy);
          md |= ok ? (1u << i) : 0u;
        }
      }
      inbx[SET] = mx; inbd[SET] = md;
    };
    auto convert = [&](int tc, int buf, auto S) {
      constexpr int SET = decltype(S)::value;
      float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
      if (has_norm && cval) {
        const int n = tc / tiles_sp;
        sc = *reinterpret_cast<const float4*>(a.in_scale + (int64_t)n * g.Cin + c);
        sh = *reinterpret_cast<const float4*>(a.in_shift + (int64_t)n * g.Cin + c);
      }
      float4 dsc = make_float4(1.f, 1.f, 1.f, 1.f);
      if (a.dy_scale) dsc = *reinterpret_cast<const float4*>(a.dy_scale + (int64_t)(tc / tiles_sp) * g.Cout + c);
      unsigned short* xh = lds + buf * (L::BUFB / 2);
      unsigned short* xl = xh + L::XLO / 2;
      unsigned short* dh = xh + L::DY / 2;
      unsigned short* dl = dh + L::DLO / 2;
      const unsigned mx = inbx[SET], md = inbd[SET];
      const unsigned fullx = last_ok ? ((1u << W16_XS) - 1u) : ((1u << (W16_XS - 1)) - 1u);
      const unsigned fulld = dlast_ok ? ((1u << W16_DS) - 1u) : ((1u << (W16_DS - 1)) - 1u);
      // specialised on two wave-uniform facts (cf. conv16_kernel): PLAIN = no norm/activation, ALLIN = nothing out of bounds
      auto body = [&](auto PL, auto AI) {
        constexpr bool PLAIN = decltype(PL)::value, ALLIN = decltype(AI)::value;
#pragma unroll
        for (int i = 0; i < W16_XS; ++i) {
          if (i == W16_XS - 1 && !last_ok) continue;
          const float4 val = px[SET][i];
          float v0 = val.x, v1 = val.y, v2 = val.z, v3 = val.w;
          if (!PLAIN) {
            v0 = fmaxf(fmaf(v0, sc.x, sh.x), fmaf(v0, sc.x, sh.x) * sl); v1 = fmaxf(fmaf(v1, sc.y, sh.y), fmaf(v1, sc.y, sh.y) * sl);
            v2 = fmaxf(fmaf(v2, sc.z, sh.z), fmaf(v2, sc.z, sh.z) * sl); v3 = fmaxf(fmaf(v3, sc.w, sh.w), fmaf(v3, sc.w, sh.w) * sl);
          }
          uint2 h, l;
          if (X3) { split_bf16(v0, v1, h.x, l.x); split_bf16(v2, v3, h.y, l.y); } else { h.x = pack_bf16(v0, v1); h.y = pack_bf16(v2, v3); }
          if (!ALLIN) {                                  // zero padding applies after the activation
            const bool was = (mx >> i) & 1u;
            h.x = was ? h.x : 0u; h.y = was ? h.y : 0u;
            if (X3) { l.x = was ? l.x : 0u; l.y = was ? l.y : 0u; }
          }
          *reinterpret_cast<uint2*>(xh + xo[i]) = h;
          if (X3) *reinterpret_cast<uint2*>(xl + xo[i]) = l;
        }
#pragma unroll
        for (int i = 0; i < W16_DS; ++i) {
          if (i == W16_DS - 1 && !dlast_ok) continue;
          float4 val = pd[SET][i];
          val.x *= dsc.x; val.y *= dsc.y; val.z *= dsc.z; val.w *= dsc.w;
          uint2 h, l;
          if (X3) { split_bf16(val.x, val.y, h.x, l.x); split_bf16(val.z, val.w, h.y, l.y); } else { h.x = pack_bf16(val.x, val.y); h.y = pack_bf16(val.z, val.w); }
          if (!ALLIN) {
            const bool was = (md >> i) & 1u;
            h.x = was ? h.x : 0u; h.y = was ? h.y : 0u;
            if (X3) { l.x = was ? l.x : 0u; l.y = was ? l.y : 0u; }
          }
          *reinterpret_cast<uint2*>(dh + dofs[i]) = h;
          if (X3) *reinterpret_cast<uint2*>(dl + dofs[i]) = l;
        }
      };
      using T_ = std::true_type; using F_ = std::false_type;
      const bool allin = __ballot(mx != fullx || md != fulld) == 0ull;     // wave-uniform
      const bool plain = !has_norm && sl == 1.f;
      if (plain) { if (allin) body(T_{}, T_{}); else body(T_{}, F_{}); }
      else       { if (allin) body(F_{}, T_{}); else body(F_{}, F_{}); }
    };
    using S0 = std::integral_constant<int, 0>;
    // one prefetch set: tile it+1 is converted right after the barrier, then tile it+2 is requested (a second register set
    // spills at this kernel's 168-VGPR budget; measured slower)
    if (niter > 0) {
      issue(origin(first), S0{});
      convert(first, 0, S0{});
      if (niter > 1) issue(origin(first + G), S0{});
    }
    for (int it = 0; it < niter; ++it) {
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (it + 1 < niter) {
        convert(first + (it + 1) * G, (it + 1) & 1, S0{});
        if (it + 2 < niter) issue(origin(first + (it + 2) * G), S0{});
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// wgrad16d: wgrad16 on bf16 OPERAND IMAGES filled by LDS-DMA.  Both operands arrive as bf16 tensors [N][D][H][W][16] -- xa16 =
// bf16(act(IN(x))) written as a side output by the layer's own InstanceNorm-backward apply pass (which has x and its statistics in
// registers anyway), dy16 = the bf16 image of the incoming gradient written by the pass that produced it (norm.hip) -- i.e. exactly
// the values wgrad16's loaders compute per tile from the fp32 tensors (single-bf16 operand products; bit-identical operands).
// What that buys (profiles/round3_conv16s_wgrad_pmc.txt: wgrad16 moves 1.9x its algorithmic bytes from L2 and is bound by one
// tile of register-staged loads in flight per CU, 26 GB/s per CU at the step's 128 workgroups):
//   * half the bytes (32 B per voxel and operand instead of 64);
//   * no conversion, no registers: the six loader waves only issue global_load_lds_dwordx4 pieces (1 KiB of LDS each, 33 per tile),
//     so THREE tiles are in flight per CU in a four-buffer LDS ring behind counted vmcnt waits and one raw s_barrier per tile;
//   * zero padding = out-of-range lanes read a 16-byte zero page.
// LDS image = wgrad16's (voxel-major rows padded to 20 voxels = 640 B = 40 granules of 16 B: conflict-free transposed reads); a
// piece is 64 consecutive granules, per-lane source address; pad granules read the zero page.  MFMA waves: wgrad16's.
// ---------------------------------------------------------------------------------------------------
#define W16D_LW 6                                       // loader waves
// arguments of wgrad16d_kernel, and what wgrad_s1d_kernel's (Ws1dArgs) share with them
struct W16dArgs {
  const uint4* xa; const uint4* dy; const uint4* zero; float* partial;
  int N, D, H, W, tiles_d, tiles_h, tiles_w, total_tiles;
  int64_t slab_floats;
};

// The loader waves of the image kernels: nothing but LDS-DMA.  A piece is 64 consecutive 16-byte granules of LDS filled by one
// global_load_lds_dwordx4 with a per-lane source address; pad granules and voxels outside the volume read the zero page.  Pieces
// 0 .. XP-1 are the x image (WgXImage: 36 rows x 40 granules), pieces XP .. XP+DPC-1 the dy image; loader wave lw issues pieces
// lw, lw + LW, ...: NI of them, a compile-time count that the vmcnt immediates need.  Tile `it` goes to buffer it & 3.
// What a kernel brings is the policy P:
//   P::L, P::LW, P::DPC     LDS layout, loader waves, pieces of the dy image
//   p.a                     the kernel's arguments (W16dArgs)
//   p.gx, p.gd, p.xg0       16-byte granules per voxel of xa16 / dy16; first granule of the workgroup's 16-channel chunk
//   p.tile(it)              the workgroup's tile walk
//   p.dy_piece(m, lane, ..) granule `lane` of dy piece m -> M-tile row (c0, c1), voxel w, granule g of that voxel, valid (no pad)
//   P::dy_dst(m)            LDS byte offset of dy piece m in its buffer
typedef __attribute__((address_space(3))) void* lds_vp;
typedef __attribute__((address_space(1))) const void* glb_vp;
template <int NI, class P>
__device__ __forceinline__ void wgrad_dma_run(const P& p, unsigned lds_base, int lw, int lane, int niter) {
  using L = typename P::L;
  static_assert(L::NBUF == 4, "three tiles in flight, one being read");
  constexpr int GPR = 2 * L::XW;                         // granules per x-image row
  const auto& a = p.a;
  const int tiles_sp = a.tiles_d * a.tiles_h * a.tiles_w;
  int off[NI]; unsigned crd[NI];                         // granule offset from the tile's operand origin; (c0, c1, w, valid)
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int s = lw + P::LW * k;                        // (wave-uniform)
    int c0, c1, w, g, gv; bool valid;
    if (s < L::XP) {
      const int gi = 64 * s + lane;
      const int row = gi / GPR, gr = gi % GPR;
      c0 = row / 6; c1 = row % 6; w = gr >> 1; g = p.xg0 + (gr & 1); gv = p.gx;
      valid = row < 36 && gr < 36;
    } else {
      p.dy_piece(s - L::XP, lane, c0, c1, w, g, valid); gv = p.gd;
    }
    off[k] = ((c0 * a.H + c1) * a.W + w) * gv + g;
    crd[k] = (unsigned)c0 | ((unsigned)c1 << 3) | ((unsigned)w << 6) | (valid ? 1u << 11 : 0u);
  }
  auto issue = [&](int it) __attribute__((always_inline)) {
    const TileOrigin o = tile_origin(p.tile(it), tiles_sp, a.tiles_h, a.tiles_w);
    const int64_t vd = (((int64_t)o.n * a.D + o.od0) * a.H + o.oh0) * a.W + o.ow0;     // voxel index of the dy tile origin
    const int64_t vx = vd - ((int64_t)a.H + 1) * a.W - 1;                              // ... of the x halo origin (-1, -1, -1)
    const unsigned lbuf = lds_base + (unsigned)(it & 3) * L::BUFB;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int s = lw + P::LW * k;
      const bool isd = s >= L::XP;
      const int c0 = (int)(crd[k] & 7u), c1 = (int)((crd[k] >> 3) & 7u), w = (int)((crd[k] >> 6) & 31u);
      const int gd = (isd ? o.od0 : o.od0 - 1) + c0, gh = (isd ? o.oh0 : o.oh0 - 1) + c1, gw = (isd ? o.ow0 : o.ow0 - 1) + w;
      const bool ok = (crd[k] >> 11) != 0u && (unsigned)gd < (unsigned)a.D && (unsigned)gh < (unsigned)a.H && (unsigned)gw < (unsigned)a.W;
      const uint4* src = (isd ? a.dy + vd * p.gd : a.xa + vx * p.gx) + off[k];
      src = ok ? src : a.zero;
      const unsigned dst = isd ? P::dy_dst(s - L::XP) : (unsigned)s * 1024u;
      __builtin_amdgcn_global_load_lds((glb_vp)src, (lds_vp)(uintptr_t)(lbuf + dst), 16, 0, 0);
    }
  };
  if (niter > 0) issue(0);
  if (niter > 1) issue(1);
  if (niter > 2) issue(2);
  for (int it = 0; it < niter; ++it) {
    // tile `it` has landed once all but the pieces of the (at most two) younger tiles in flight are done
    if (it + 2 < niter) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * NI) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    if (it + 3 < niter) issue(it + 3);                   // into the buffer the MFMA waves finished before this barrier
  }
}
template <class P>
__device__ __forceinline__ void wgrad_dma_loader(const P& p, unsigned lds_base, int lw, int lane, int niter) {
  constexpr int NP = P::L::XP + P::DPC;
  if (lw < NP % P::LW) wgrad_dma_run<NP / P::LW + 1>(p, lds_base, lw, lane, niter);
  else wgrad_dma_run<NP / P::LW>(p, lds_base, lw, lane, niter);
}

struct W16dDma {
  using L = W16Lds<false, true>;
  static constexpr int LW = W16D_LW, DPC = L::DPC;
  static constexpr int gx = 2, gd = 2, xg0 = 0;          // 16 channels: two granules per voxel, one chunk
  const W16dArgs& a; int first, G;
  __device__ int tile(int it) const { return first + it * G; }
  __device__ void dy_piece(int m, int lane, int& c0, int& c1, int& w, int& g, bool& valid) const {   // rows of 40 granules, like x
    const int gi = 64 * m + lane, row = gi / 40, gr = gi % 40;
    c0 = row >> 2; c1 = row & 3; w = gr >> 1; g = gr & 1; valid = gr < 32;
  }
  static __device__ constexpr unsigned dy_dst(int m) { return L::DY + (unsigned)m * 1024u; }
};

__global__ __launch_bounds__(256 + 64 * W16D_LW) void wgrad16d_kernel(const W16dArgs a) {
  extern __shared__ float4 lds4[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = (int)gridDim.x, per = G >> 3;
  const int first = (blockIdx.x & 7) * per + (blockIdx.x >> 3);      // tile(it) = first + it * G   (XCD-aware, see wgrad16_kernel)
  const int niter = first < a.total_tiles ? (a.total_tiles - first + G - 1) / G : 0;
  const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds4;
  if (wave < 4)
    wgrad16_mfma<W16dDma::L>(lds_base, wave, lane, niter, reinterpret_cast<float4*>(a.partial + (int64_t)blockIdx.x * a.slab_floats));
  else
    wgrad_dma_loader(W16dDma{a, first, G}, lds_base, wave - 4, lane, niter);
}

// ---------------------------------------------------------------------------------------------------
// wgrad_s1: the 3x3x3 stride-1 layers the generic kernel above used to take (32 / 64 / 128 channels; 38 launches per step, the
// largest single item of the step's kernel time), single-bf16 operands, restructured like wgrad16_kernel.  The generic kernel
// stages a tile with one DEPENDENT global load per staging slot (11 x slots + CGW/4 dy slots per thread: load, wait, convert,
// store, next) and only then starts its MFMA phase: ~19 exposed round trips per tile, 4.6 us against 0.75 us of MFMAs
// (32 ch @ 64^3: 111 us per launch under rocprofv3, tools/wgrad_micro.py).  Here a workgroup is 12 waves, one per CU:
//   * waves 4-11 (loaders) convert tile t+1 (recomputed InstanceNorm + activation for x) into the OTHER LDS buffer, then issue ALL
//     loads of tile t+3 (straight-line, masked by pointer select) into the register set that frees: two tiles of loads in flight
//     (eight loader waves keep a set at 8-10 float4 per thread; with four, two sets spill and one set is latency-bound: 59 us);
//   * waves 0-3 (MFMA) run the 56-step transposed-read / MFMA phase of tile t (wave w owns taps w, w+4, ...; slot 27 = bias row)
//     with accumulators persistent over the workgroup's whole tile range;
//   * one raw s_barrier per tile hands the buffers over; one slab per workgroup, fewer and longer workgroups than the generic
//     plan (256 in all), so the slab traffic and the reduce halve as well.
// Same (chunk, channel-group) blocking, LDS image layout (padded / skewed rows: conflict-free transposed reads) and slab layout
// as wgrad_bf16_kernel<7, NTW, true, false>.  Measured (slab kernel, rocprofv3): 32 ch @ 64^3 111 -> 50 us, 64 ch @ 32^3 60 -> 28 us,
// 128 ch @ 16^3 37 -> 22 us.  At 50 us the (tile, chunk) units move 300 MB of L2 -> CU traffic (x halo 41 KB + dy 32 KB each;
// 2.2x the 134 MB the layer reads from HBM) = 6.0 TB/s -- the same aggregate ingest rate wgrad16_kernel sits at (934 MB in
// 150 us), i.e. the CU <- L2 fabric, not the MFMA phase (a deeper LDS-read lookahead changed nothing).  What is left is traffic:
// both chunks of a tile against one dy fetch, a sliding halo.
// ---------------------------------------------------------------------------------------------------
#define WS1_LW 8                                        // loader waves (MFMA waves: 4) -> 768-thread workgroups
// LDS layout of the wgrad_s1 pair, one definition for kernels and launchers.  A buffer is x image | dy image.  The dy image is 16
// M-tile rows of 16 voxels x CGW channels in the generic kernel's form (wg_dy_pitch / wg_dy_skew): row m starts at element
// m * DP * CGW + ((m + 1) >> 1) * DSK.  DMA = false: two buffers written by converting loader waves (wgrad_s1_kernel<NTW>);
// DMA = true: a four-buffer ring filled by LDS-DMA (wgrad_s1d_kernel), where one row of 32 channels is one piece.  Offsets in bytes.
template <int NTW_, bool DMA> struct Ws1Lds : WgXImage {
  static constexpr int NTW = NTW_, CGW = NTW * 16;
  static constexpr int DP = wg_dy_pitch(CGW), DSK = wg_dy_skew(CGW);
  static constexpr int DSLOTS = DMA ? 8 : 16 / 2 + 1;                    // skews allotted: row 15 carries 8, the generic form allots MT / 2 + 1
  static constexpr unsigned DIB = (16 * DP * CGW + DSLOTS * DSK) * 2u;   // bytes of the dy image
  static constexpr unsigned DY = DMA ? XP * 1024u : XI * 2u;             // dy image = bytes the x image takes
  static constexpr unsigned BUFB = DY + DIB;                             // buffer pitch (DMA: 40,192 B)
  static constexpr int NBUF = DMA ? 4 : 2;
  static constexpr size_t BYTES = (size_t)NBUF * BUFB;                   // dynamic LDS of a launch
  static_assert((NTW == 1 || NTW == 2) && BUFB % 16 == 0 && (!DMA || DP * CGW * 2 == 1024), "wgrad_s1 layout");
};

// MFMA waves (0-3) of the wgrad_s1 pair.  L: the pair's LDS layout (NTW, dy pitch and skew, image offset, buffer pitch and count);
// out: the (chunk, group) block of the workgroup's slab, [tap slot 0..27][tile j][lane][4] (layout of wgrad_bf16_kernel).
template <class L>
__device__ __forceinline__ void wgrad_s1_mfma(unsigned lds_base, int wave, int lane, int niter, float4* out) {
  constexpr int NTW = L::NTW, CGW = L::CGW, XW = L::XW, DP = L::DP, DSK = L::DSK;
  const int kq = lane >> 4, bq = (lane & 15) >> 2, bp = lane & 3;
  f32x4 acc[7][NTW];
#pragma unroll
  for (int i = 0; i < 7; ++i)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const bf16x8 ones = ones_frag();
  const bool bias_wave = wave == 3;
  const unsigned lane_x = lds_base + (((kq & 1) * XW + (kq >> 1) * 8 + bq) * 16 + bp * 4) * 2;
  unsigned xa0[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int t = wave + 4 * i;
    xa0[i] = lane_x + (t < 27 ? (((t / 9) * 6 + (t / 3) % 3) * XW + t % 3) * 32 : 0);
  }
  const unsigned da0 = lds_base + L::DY + (((kq & 1) * DP + (kq >> 1) * 8 + bq) * CGW + (kq & 1) * DSK + bp * 4) * 2;
  for (int it = 0; it < niter; ++it) {
    asm volatile("s_barrier" ::: "memory");              // buffer it & (NBUF - 1) is complete
    const unsigned bo = (unsigned)(it & (L::NBUF - 1)) * L::BUFB;
    unsigned xa[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) xa[i] = xa0[i] + bo;
    const unsigned da = da0 + bo;
    constexpr int DEPTH = WS1_DEPTH;                   // tap steps of LDS-read lookahead (a step is NTW MFMAs = 16-32 cycles)
    bf16x8 ah[DEPTH + 1], bh[2][NTW];
    auto issue = [&](int f) __attribute__((always_inline)) {   // f = ks * 7 + i, compile-time after unrolling
      const int ks = f / 7, i = f % 7;
      if (i == 0) {
        const unsigned od_ = (2 * ks * DP * CGW + ks * DSK) * 2;
#pragma unroll
        for (int j = 0; j < NTW; ++j) bh[ks & 1][j] = tr_frag_at(da + od_ + j * 32, 4 * CGW * 2);
      }
      const unsigned ox = (((ks >> 1) * 6 + ((2 * ks) & 3)) * XW) * 32;
      ah[f % (DEPTH + 1)] = tr_frag_at(xa[i] + ox, 4 * 32);
    };
#pragma unroll
    for (int f = 0; f < DEPTH; ++f) issue(f);
#pragma unroll
    for (int f = 0; f < 56; ++f) {
      if (f + DEPTH < 56) issue(f + DEPTH);
      __builtin_amdgcn_sched_barrier(0);
      const int ks = f / 7, i = f % 7;
      bf16x8 ahf = ah[f % (DEPTH + 1)];
      if (i == 6) ahf = bias_wave ? ones : ahf;            // wave 3: tap slot 27 = bias row (ones . dy); wave-uniform select
#pragma unroll
      for (int j = 0; j < NTW; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahf, bh[ks & 1][j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int t = wave + 4 * i;
    if (t > 27) continue;
#pragma unroll
    for (int j = 0; j < NTW; ++j)
      out[((int64_t)t * NTW + j) * 64 + lane] = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
  }
}

template <int NTW>
__global__ __launch_bounds__(256 + 64 * WS1_LW) void wgrad_s1_kernel(const WgArgsB a) {
  using L = Ws1Lds<NTW, false>;
  constexpr int CGW = L::CGW, XW = L::XW, DP = L::DP, DSK = L::DSK;
  extern __shared__ float4 lds4[];
  const ConvGeom& g = a.g;
  unsigned short* lds = reinterpret_cast<unsigned short*>(lds4);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int split = blockIdx.x;
  const int chunk = blockIdx.y / a.ngroups, grp = blockIdx.y % a.ngroups;
  const float* ax_ = a.groups ? a.x_g[blockIdx.z] : a.x;             // (workgroup-uniform: group operands of a grouped launch)
  const float* ady_ = a.groups ? a.dy_g[blockIdx.z] : a.dy;
  float* apart_ = a.groups ? a.partial_g[blockIdx.z] : a.partial;
  const int co0 = grp * CGW;
  const int tiles_sp = g.tiles_d * g.tiles_h * g.tiles_w;
  const int t_begin = split * a.tiles_per_split;
  const int t_end = min(a.total_tiles, t_begin + a.tiles_per_split);
  const int niter = max(t_end - t_begin, 0);

  if (wave < 4) {
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds4;
    float4* slab = reinterpret_cast<float4*>(apart_ + (int64_t)split * a.slab_floats);
    wgrad_s1_mfma<L>(lds_base, wave, lane, niter, slab + ((int64_t)chunk * a.ngroups + grp) * (28 * NTW * 64));
  } else {
    // =============================================================== loader waves
    const int lt = tid - 256;
    constexpr int LT = 64 * WS1_LW;                         // loader threads
    constexpr int VPP = LT / 4;                             // x voxels staged per pass (4 threads per voxel)
    constexpr int XS = (W16_NVOX + VPP - 1) / VPP;              // 6 x staging slots per loader thread
    constexpr int DSL = CGW / 4;                            // channel quads per dy voxel
    constexpr int DS = 256 * DSL / LT;                      // 2 (16 output channels) or 4 (32) dy staging slots per loader thread
    constexpr int DROWS = LT / DSL / 16;                    // M-tile rows covered by one dy slot over all loader threads
    static_assert(256 * DSL % LT == 0 && LT / DSL % 16 == 0, "dy slots are whole M-tile rows");
    const int q = lt & 3;
    const int c = chunk * 16 + q * 4;
    const bool cval = c < g.Cin;
    const bool has_norm = a.in_scale != nullptr;
    const bool plain = !has_norm && a.in_slope == 1.f;
    int relx[XS];
    unsigned xo[XS];                                        // LDS element offset | (idd, ih, iw) << 16 (bounds tests per tile)
#pragma unroll
    for (int i = 0; i < XS; ++i) {
      int v = (lt >> 2) + VPP * i; if (v > 647) v = 647;    // (last slot: 8 real voxels; the rest re-read the last one)
      const int iw = v % 18, t2 = v / 18, ih = t2 % 6, idd = t2 / 6;
      relx[i] = ((idd * g.Hi + ih) * g.Wi + iw) * g.x_ldc + c;
      xo[i] = (unsigned)((t2 * XW + iw) * 16 + q * 4) | ((unsigned)idd << 16) | ((unsigned)ih << 19) | ((unsigned)iw << 22);
    }
    // dy slot k of this thread: element e = lt + LT k -> voxel e / DSL, channel quad e % DSL: slot k is slot 0 moved by DROWS whole
    // M-tile rows -- per-thread base + wave-uniform increments
    const int vox0 = lt / DSL, cq0 = lt % DSL, m0 = vox0 >> 4, tw = vox0 & 15;
    const int reld0 = (((m0 >> 2) * g.Ho + (m0 & 3)) * g.Wo + tw) * a.dy_ldc + co0 + cq0 * 4;
    const bool last_x = (lt >> 2) + VPP * (XS - 1) < W16_NVOX; // the last slot holds a real voxel for this thread
    const bool co_ok = co0 + cq0 * 4 < g.Cout;
    // TWO register sets of loads in flight (a tile period is shorter than one memory round trip under load); eight loader waves
    // keep a set at XS + DS = 8..10 float4 per thread
    float4 vx[2][XS], vd[2][DS], sc[2], sh[2];
    unsigned okx[2] = {0u, 0u}, okd[2] = {0u, 0u};
    sc[0] = sc[1] = make_float4(1.f, 1.f, 1.f, 1.f); sh[0] = sh[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    auto issue = [&](int tile, auto S) __attribute__((always_inline)) {
      constexpr int SET = decltype(S)::value;
      const TileOrigin o = tile_origin(tile, tiles_sp, g.tiles_h, g.tiles_w);
      const int n = o.n, od0 = o.od0, oh0 = o.oh0, ow0 = o.ow0;
      const int id0 = od0 - 1, ih0 = oh0 - 1, iw0 = ow0 - 1;
      const float* xb = ax_ + ((((int64_t)n * g.Di + id0) * g.Hi + ih0) * g.Wi + iw0) * g.x_ldc;
      const float* db = ady_ + ((((int64_t)n * g.Do + od0) * g.Ho + oh0) * g.Wo + ow0) * a.dy_ldc;
      if (has_norm && cval) {
        sc[SET] = *reinterpret_cast<const float4*>(a.in_scale + (int64_t)n * g.Cin + c);
        sh[SET] = *reinterpret_cast<const float4*>(a.in_shift + (int64_t)n * g.Cin + c);
      }
      unsigned mx = 0, md = 0;
#pragma unroll
      for (int i = 0; i < XS; ++i) {
        const int gd = id0 + (int)((xo[i] >> 16) & 7u), gh = ih0 + (int)((xo[i] >> 19) & 7u), gw = iw0 + (int)(xo[i] >> 22);
        const bool ok = cval && (i < XS - 1 || last_x) && (unsigned)gd < (unsigned)g.Di && (unsigned)gh < (unsigned)g.Hi && (unsigned)gw < (unsigned)g.Wi;
        vx[SET][i] = *reinterpret_cast<const float4*>(ok ? xb + relx[i] : ax_);      // unconditional load, masked at conversion
        mx |= ok ? (1u << i) : 0u;
      }
#pragma unroll
      for (int k = 0; k < DS; ++k) {
        const int m = m0 + k * DROWS;
        const bool ok = co_ok && od0 + (m >> 2) < g.Do && oh0 + (m & 3) < g.Ho && ow0 + tw < g.Wo;
        const int rel = reld0 + ((((m >> 2) - (m0 >> 2)) * g.Ho + ((m & 3) - (m0 & 3))) * g.Wo) * a.dy_ldc;
        vd[SET][k] = *reinterpret_cast<const float4*>(ok ? db + rel : ady_);
        md |= ok ? (1u << k) : 0u;
      }
      okx[SET] = mx; okd[SET] = md;
    };
    auto commit = [&](int buf, auto S) __attribute__((always_inline)) {
      constexpr int SET = decltype(S)::value;
      unsigned short* xh = lds + (buf ? L::BUFB / 2 : 0);
      unsigned short* dh = xh + L::DY / 2;
#pragma unroll
      for (int i = 0; i < XS; ++i) {
        if (i == XS - 1 && !last_x) continue;
        float4 val = vx[SET][i];
        if (!plain) {
          val.x = cwf_act(val.x * sc[SET].x + sh[SET].x, a.in_slope); val.y = cwf_act(val.y * sc[SET].y + sh[SET].y, a.in_slope);
          val.z = cwf_act(val.z * sc[SET].z + sh[SET].z, a.in_slope); val.w = cwf_act(val.w * sc[SET].w + sh[SET].w, a.in_slope);
        }
        uint2 h; h.x = pack_bf16(val.x, val.y); h.y = pack_bf16(val.z, val.w);
        const bool was = (okx[SET] >> i) & 1u;              // zero padding applies after the activation
        h.x = was ? h.x : 0u; h.y = was ? h.y : 0u;
        *reinterpret_cast<uint2*>(xh + (xo[i] & 0xffffu)) = h;
      }
#pragma unroll
      for (int k = 0; k < DS; ++k) {
        const int m = m0 + k * DROWS;
        const float4 val = vd[SET][k];
        uint2 h; h.x = pack_bf16(val.x, val.y); h.y = pack_bf16(val.z, val.w);
        const bool was = (okd[SET] >> k) & 1u;
        h.x = was ? h.x : 0u; h.y = was ? h.y : 0u;
        *reinterpret_cast<uint2*>(dh + (m * DP + tw) * CGW + ((m + 1) >> 1) * DSK + cq0 * 4) = h;
      }
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    // tile u lives in register set u & 1 and LDS buffer u & 1.  Iteration it: tile it+1 is converted right after the barrier, then
    // tile it+3 is requested into the set it frees (tile it+2 is already in flight in the other set)
    if (niter > 0) {
      issue(t_begin, S0{});
      commit(0, S0{});
      if (niter > 1) issue(t_begin + 1, S1{});
      if (niter > 2) issue(t_begin + 2, S0{});
    }
    for (int it = 0; it < niter; it += 2) {
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (it + 1 < niter) {
        commit(1, S1{});
        if (it + 3 < niter) issue(t_begin + it + 3, S1{});
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (it + 2 < niter) {
          commit(0, S0{});
          if (it + 4 < niter) issue(t_begin + it + 4, S0{});
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// wgrad_s1d: wgrad_s1 (32-channel output groups) on bf16 OPERAND IMAGES filled by LDS-DMA -- the wgrad16d recipe for the 32 / 64 / 128-
// channel 3x3x3 stride-1 layers: xa16 [N][D][H][W][Cin] and dy16 [N][D][H][W][Cout] bf16 (written by the InstanceNorm-backward apply
// passes / block tails, or by cwf_to_bf16), eight loader waves issue nothing but global_load_lds_dwordx4 pieces -- 23 for the x image of
// the workgroup's 16-channel chunk (wgrad16d's), 16 for the dy image (one M-tile row of 16 voxels x 32 channels IS one 1-KiB piece;
// the 32-byte skew of odd rows moves the piece's base) -- into a four-buffer ring, three tiles in flight.  MFMA waves, slab layout
// and (chunk, group) blocking: wgrad_s1_kernel<2>.  (wgrad_s1 moves 3.3-3.5x its algorithmic bytes from L2 as fp32; this form
// moves the same halo-amplified voxels at half the bytes, without conversion work and with three tiles of latency cover.)
// ---------------------------------------------------------------------------------------------------
struct Ws1dArgs : W16dArgs { int Cin, Cout, tiles_per_split, ngroups; };

struct Ws1dDma {
  using L = Ws1Lds<2, true>;
  static constexpr int LW = WS1_LW, DPC = 16;
  const Ws1dArgs& a; int gx, gd, xg0, dg0, t_begin;     // dg0: first granule of the workgroup's 32-channel group
  __device__ int tile(int it) const { return t_begin + it; }
  __device__ void dy_piece(int m, int lane, int& c0, int& c1, int& w, int& g, bool& valid) const {   // M-tile row m: 16 voxels x 4 granules
    c0 = m >> 2; c1 = m & 3; w = lane >> 2; g = dg0 + (lane & 3); valid = true;
  }
  static __device__ constexpr unsigned dy_dst(int m) { return L::DY + (unsigned)(m * 1024 + ((m + 1) >> 1) * 32); }   // (skewed rows)
};

__global__ __launch_bounds__(256 + 64 * WS1_LW) void wgrad_s1d_kernel(const Ws1dArgs a) {
  using L = Ws1dDma::L;
  extern __shared__ float4 lds4[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int split = blockIdx.x;
  const int chunk = blockIdx.y / a.ngroups, grp = blockIdx.y % a.ngroups;
  const int t_begin = split * a.tiles_per_split;
  const int t_end = min(a.total_tiles, t_begin + a.tiles_per_split);
  const int niter = max(t_end - t_begin, 0);
  const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds4;
  if (wave < 4) {
    float4* slab = reinterpret_cast<float4*>(a.partial + (int64_t)split * a.slab_floats);
    wgrad_s1_mfma<L>(lds_base, wave, lane, niter, slab + ((int64_t)chunk * a.ngroups + grp) * (28 * L::NTW * 64));
  } else {
    wgrad_dma_loader(Ws1dDma{a, a.Cin >> 3, a.Cout >> 3, chunk * 2, grp * 4, t_begin}, lds_base, wave - 4, lane, niter);
  }
}

// ---------------------------------------------------------------------------------------------------
// pw_wgrad: weight gradients of the pointwise family (1x1x1 convs; ConvTranspose k = 2, s = 2), the counterpart of pw_conv_kernel
// (conv_bf16.hip).  dW[ci][co] = sum_vox xa[vox][ci] * dy[vox][co] is a skinny product over a pure stream -- x and dy are each read
// once, ~0.5 FLOP per byte -- and the generic 1-tap path above (stage a 256-voxel tile in LDS, barrier, transposed reads, barrier;
// one launch block per 16-channel chunk, so dy is re-read per chunk) ran it at 10-28 % of the HBM rate (1x1 32->16 @128^3: 366 us
// for 805 MB with its reduce; tools/layer_table.py).  Here there is no LDS staging and no barrier in the loop:
//   * v_mfma_f32_16x16x4_f32 contracts FOUR voxels per instruction, one fp32 value per lane: lane (i, k) of the A operand is
//     x[voxel k][channel i], of the B operand dy[voxel k][channel j] -- exactly what a dword load of 16 consecutive channels x 4
//     consecutive voxels hands the wave, so fragments come straight from global memory (exact fp32 products: no bf16 rounding);
//   * a wave owns a contiguous run of 4-voxel groups of ONE sample and ALL (chunk, tile) blocks of the layer: x and dy are read
//     exactly once; the loads of G groups are issued together (dword loads: 256 B per instruction, so many must be in flight);
//   * InstanceNorm + activation of x recomputed in registers; bias row = ones operand, as in the tiled kernels;
//   * the 8 or 16 waves of a workgroup sum their accumulators through LDS: one slab per workgroup (256 in all: the slab reduce
//     walks the slabs serially per element, 1024 of them cost it 84 us), in the generic slab layout.
// ---------------------------------------------------------------------------------------------------
struct PwWgWork { int Vin, gps, wps, gpw; };            // input voxels per sample, 4-voxel groups per sample, workgroups per sample, groups per wave

// waves per workgroup (one workgroup per CU): 16 where the accumulators leave room (<= 128 VGPRs), else 8
template <int NCH, int NTL, int NCLS> struct PwgCfg { static constexpr int WAVES = (NCLS * NTL * (NCH + 1) <= 12) ? 16 : 8; };
template <int NCH, int NTL, int NCLS>
__global__ __launch_bounds__((64 * PwgCfg<NCH, NTL, NCLS>::WAVES)) void pw_wgrad_kernel(const WgArgsB a, const PwWgWork wk, int CG) {
  constexpr int PWG_WAVES = PwgCfg<NCH, NTL, NCLS>::WAVES, RB = 32 / PWG_WAVES;      // RB: blocks per reduction round
  constexpr int G = (NCLS > 1) ? (NCH * NTL > 1 ? 1 : 2) : (NCH + NTL <= 2 ? 16 : (NCH + NTL <= 3 ? 12 : (NCH + NTL <= 6 ? 4 : 2)));   // groups per iteration
  __shared__ float4 red[PWG_WAVES][RB][64];
  const ConvGeom& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = (int)blockIdx.x / wk.wps, wg = (int)blockIdx.x % wk.wps;
  const int gA = (wg * PWG_WAVES + wave) * wk.gpw;
  const int gB = min(gA + wk.gpw, wk.gps);
  const float* xs = a.x + (int64_t)n * wk.Vin * g.x_ldc;
  const float* ds = a.dy + (int64_t)n * g.Do * g.Ho * g.Wo * a.dy_ldc;
  const bool has_norm = a.in_scale != nullptr;
  const bool plain = !has_norm && a.in_slope == 1.f;
  float sc[NCH], sh[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ci = c * 16 + li;
    sc[c] = (has_norm && ci < g.Cin) ? a.in_scale[(int64_t)n * g.Cin + ci] : 1.f;
    sh[c] = (has_norm && ci < g.Cin) ? a.in_shift[(int64_t)n * g.Cin + ci] : 0.f;
  }
  f32x4 acc[NCLS][NCH][NTL], accb[NCLS][NTL];
#pragma unroll
  for (int q = 0; q < NCLS; ++q)
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
      accb[q][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NCH; ++c) acc[q][c][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

  for (int gi = gA; gi < gB; gi += G) {
    float xv[G][NCH], dv[G][NCLS][NTL];
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const bool ok = gi + k < gB;                          // wave-uniform
      const int vox = (gi + k) * 4 + lk;                    // this lane's voxel of the group
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int ci = c * 16 + li;
        xv[k][c] = (ok && ci < g.Cin) ? xs[(int64_t)vox * g.x_ldc + ci] : 0.f;
      }
      int64_t ov[NCLS];
      if (NCLS == 1) ov[0] = vox;
      else {
        const int w_ = vox % g.Wi, t2 = vox / g.Wi, h_ = t2 % g.Hi, d_ = t2 / g.Hi;
#pragma unroll
        for (int q = 0; q < NCLS; ++q) ov[q < NCLS ? q : 0] = ((int64_t)(2 * d_ + (q >> 2)) * g.Ho + 2 * h_ + ((q >> 1) & 1)) * g.Wo + 2 * w_ + (q & 1);
      }
#pragma unroll
      for (int q = 0; q < NCLS; ++q)
#pragma unroll
        for (int t = 0; t < NTL; ++t) {
          const int co = t * 16 + li;
          dv[k][q][t] = (ok && co < g.Cout) ? ds[ov[q] * a.dy_ldc + co] : 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const bool ok = gi + k < gB;
      float xa[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        float v = xv[k][c];
        if (!plain) v = cwf_act(v * sc[c] + sh[c], a.in_slope);
        xa[c] = (ok && c * 16 + li < g.Cin) ? v : 0.f;      // (a masked lane would otherwise carry act(shift))
      }
#pragma unroll
      for (int q = 0; q < NCLS; ++q)
#pragma unroll
        for (int t = 0; t < NTL; ++t) {
          accb[q][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.f, dv[k][q][t], accb[q][t], 0, 0, 0);
#pragma unroll
          for (int c = 0; c < NCH; ++c) acc[q][c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[c], dv[k][q][t], acc[q][c][t], 0, 0, 0);
        }
    }
  }

  // ---- one slab per workgroup: block (class, chunk, group, tap 0 = weights / 1 = bias row, tile) = 64 lanes x float4.
  // The waves' accumulators meet in LDS RB blocks at a time; waves 0..RB-1 each sum one block over all waves and store it.
  float4* out = reinterpret_cast<float4*>(a.partial + (int64_t)blockIdx.x * a.slab_floats);
  constexpr int NB = NCLS * NTL * (NCH + 1);
  f32x4 flat[NB]; int bid[NB];
  {
    int u = 0;
#pragma unroll
    for (int q = 0; q < NCLS; ++q)
#pragma unroll
      for (int t = 0; t < NTL; ++t) {
        const int grp = t / CG, j = t % CG;
#pragma unroll
        for (int c = 0; c < NCH; ++c) { flat[u] = acc[q][c][t]; bid[u] = a.cls_slab_base[q] + ((c * a.ngroups + grp) * 2) * CG + j; ++u; }
        // tap slot 1: the all-ones row.  Every chunk's slot is written (the reduce map reads chunk 0's), as in the tiled kernel
        flat[u] = accb[q][t]; bid[u] = a.cls_slab_base[q] + ((0 * a.ngroups + grp) * 2 + 1) * CG + j; ++u;
      }
  }
#pragma unroll
  for (int b0 = 0; b0 < NB; b0 += RB) {
    __syncthreads();
#pragma unroll
    for (int r_ = 0; r_ < RB; ++r_)
      if (b0 + r_ < NB) red[wave][r_][lane] = make_float4(flat[b0 + r_][0], flat[b0 + r_][1], flat[b0 + r_][2], flat[b0 + r_][3]);
    __syncthreads();
    if (wave < RB && b0 + wave < NB) {
      float4 sum = red[0][wave][lane];
#pragma unroll
      for (int w = 1; w < PWG_WAVES; ++w) { const float4 p = red[w][wave][lane]; sum.x += p.x; sum.y += p.y; sum.z += p.z; sum.w += p.w; }
      int id = bid[b0];
#pragma unroll
      for (int r_ = 1; r_ < RB; ++r_) if (b0 + r_ < NB && wave == r_) id = bid[b0 + r_];
      out[(int64_t)id * 64 + lane] = sum;
      if (NCH > 1) {                                        // the bias rows of chunks 1.. (same values)
#pragma unroll
        for (int r_ = 0; r_ < RB; ++r_) {
          if (b0 + r_ < NB && wave == r_ && (b0 + r_) % (NCH + 1) == NCH) {
            for (int c = 1; c < NCH; ++c) out[((int64_t)id + (int64_t)c * a.ngroups * 2 * CG) * 64 + lane] = sum;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// host side: ONE plan per descriptor.  wgrad_bf16_plan makes every decision of a bf16-form weight-gradient launch -- argument
// checks, kernel instance, grid, tile walk, slabs written -- and fills the kernels' argument structs; wgrad_bf16_launch only
// launches what the plan says, and cwf_debug_wgrad_bf16_plan reports the same plan without launching (include/cwf_hip.h).
// The split-K plan agrees with wgrad_mfma.hip's: the caller sized the slab buffer through cwf_wgrad_nsplit / cwf_wgrad_slab_floats.
// ---------------------------------------------------------------------------------------------------
struct WgBf16Plan {
  int id;                                                 // enum cwf_wgrad_bf16_instance
  int gx, gy, gz, threads;
  size_t lds;
  int walk, walk_step, waves;                             // CWF_WGB_WALK_*; tiles_per_split / grid / groups per wave; waves sharing a pw walk
  int items, items_lo, items_hi;                          // tiles (pw: 4-voxel groups per sample) in all; fewest / most per workgroup
  int64_t slab;
  int nsplit_used;
  int exact;                                              // 1: exact fp32 products (pw_wgrad_kernel), 0: bf16 operands
  WgArgsB a; PwWgWork wk; int CG;                         // arguments of the fp32-tensor kernels
  Ws1dArgs ad;                                            // ... of the bf16-image kernels (wgrad16d_kernel takes its W16dArgs part)
};

// contiguous ranges of `tps` tiles over `total`: grid x, fewest / most tiles of a workgroup
static void wg_plan_ranges(WgBf16Plan& p, int splits, int tps, int total) {
  p.walk = CWF_WGB_WALK_RANGES; p.walk_step = tps; p.waves = 0; p.items = total;
  p.items_hi = tps < total ? tps : total; p.items_lo = total - (splits - 1) * tps;
}
// the XCD-aware strided walk of the 16 -> 16 kernels over `grid` workgroups
static void wg_plan_strided(WgBf16Plan& p, int grid, int total) {
  p.walk = CWF_WGB_WALK_STRIDED; p.walk_step = grid; p.waves = 0; p.items = total;
  p.items_lo = total / grid; p.items_hi = cdiv(total, grid);
}

// what both image kernels ask of their arguments; fills the fields the two kernels share
static int wgrad_image_args(const cwf_wgrad_args& d, W16dArgs& a) {
  if (!d.xa16 || !d.dy16 || !d.zero16 || !d.partial || d.N <= 0 || d.Di <= 0 || d.Hi <= 0 || d.Wi <= 0) return CWF_E_BADARG;
  if (((uintptr_t)d.xa16 & 15) || ((uintptr_t)d.dy16 & 15) || ((uintptr_t)d.zero16 & 15) || ((uintptr_t)d.partial & 15)) return CWF_E_ALIGN;
  a.xa = (const uint4*)d.xa16; a.dy = (const uint4*)d.dy16; a.zero = (const uint4*)d.zero16; a.partial = d.partial;
  a.N = d.N; a.D = d.Di; a.H = d.Hi; a.W = d.Wi;
  a.tiles_d = cdiv(a.D, 4); a.tiles_h = cdiv(a.H, 4); a.tiles_w = cdiv(a.W, 16);
  a.total_tiles = a.N * a.tiles_d * a.tiles_h * a.tiles_w;
  return 0;
}

static int wgrad16d_plan(const cwf_wgrad_args& d, WgBf16Plan& p) {
  W16dArgs& a = p.ad;
  if (const int rc = wgrad_image_args(d, a)) return rc;
  if ((int64_t)a.N * a.D * a.H * a.W >= (1ll << 30)) return CWF_E_TOOLARGE;
  a.slab_floats = 28 * 256;                               // = cwf_wgrad_slab_floats(CWF_CONV3_S1, 16, 16)
  int grid = SIDE_WGS; while (grid > 8 && grid > a.total_tiles) grid -= 8;      // multiple of 8 (XCD-aware tile map)
  if (grid > cwf_wgrad_nsplit(CWF_CONV3_S1, a.N, a.D, a.H, a.W, 16, 16)) return CWF_E_BADARG;    // (the caller's slab buffer is sized by it)
  p.id = CWF_WGB_WGRAD16D; p.gx = grid; p.gy = 1; p.gz = 1; p.threads = 256 + 64 * W16D_LW; p.lds = W16dDma::L::BYTES;
  wg_plan_strided(p, grid, a.total_tiles);
  p.slab = a.slab_floats; p.nsplit_used = grid; p.exact = 0;
  return 0;
}

static int wgrad_s1d_plan(const cwf_wgrad_args& d, WgBf16Plan& p) {
  const int Cin = d.Cin, Cout = d.Cout;
  Ws1dArgs& a = p.ad;
  if (const int rc = wgrad_image_args(d, a)) return rc;
  if (Cin < 16 || (Cin & 15) || Cout < 32 || (Cout & 31)) return CWF_E_BADARG;
  if ((int64_t)a.N * a.D * a.H * a.W * (Cin > Cout ? Cin : Cout) >= (1ll << 33)) return CWF_E_TOOLARGE;
  a.Cin = Cin; a.Cout = Cout;
  const int nchunks = Cin / 16;
  a.ngroups = Cout / 32;
  const int nblk = nchunks * a.ngroups;
  a.slab_floats = (int64_t)nblk * 28 * 2 * 256;
  if (a.slab_floats != cwf_wgrad_slab_floats(CWF_CONV3_S1, Cin, Cout)) return CWF_E_BADARG;
  int want = SIDE_WGS / nblk; if (want < 1) want = 1; if (want > a.total_tiles) want = a.total_tiles;
  a.tiles_per_split = cdiv(a.total_tiles, want);
  const int splits = cdiv(a.total_tiles, a.tiles_per_split);
  if (splits > cwf_wgrad_nsplit(CWF_CONV3_S1, a.N, a.D, a.H, a.W, Cin, Cout)) return CWF_E_BADARG;     // (the caller's slab buffer is sized by it)
  p.id = CWF_WGB_S1D; p.gx = splits; p.gy = nblk; p.gz = 1; p.threads = 256 + 64 * WS1_LW; p.lds = Ws1dDma::L::BYTES;
  wg_plan_ranges(p, splits, a.tiles_per_split, a.total_tiles);
  p.slab = a.slab_floats; p.nsplit_used = splits; p.exact = 0;
  return 0;
}

// pointwise stream kernel <NCH, NTL, NCLS>: false when the workspace (max_slabs slabs) cannot hold one slab per sample
template <int NCH, int NTL, int NCLS>
static bool pw_wgrad_plan(WgBf16Plan& p, int id, int max_slabs) {
  const ConvGeom& g = p.a.g;
  PwWgWork& wk = p.wk;
  wk.Vin = g.Di * g.Hi * g.Wi;
  wk.gps = wk.Vin >> 2;
  int wps = SIDE_WGS / g.N; if (wps < 1) wps = 1;        // ~one 8/16-wave workgroup per CU in all, each inside one sample
  if (wps * g.N > max_slabs) wps = max_slabs / g.N;
  if (wps < 1) return false;
  constexpr int PWG_WAVES = PwgCfg<NCH, NTL, NCLS>::WAVES;
  const int maxw = cdiv(wk.gps, PWG_WAVES * 8);
  if (wps > maxw) wps = maxw;
  wk.gpw = cdiv(wk.gps, wps * PWG_WAVES);
  wk.wps = cdiv(wk.gps, wk.gpw * PWG_WAVES);
  p.id = id; p.gx = wk.wps * g.N; p.gy = 1; p.gz = 1; p.threads = 64 * PWG_WAVES; p.lds = 0;
  p.walk = CWF_WGB_WALK_PW; p.walk_step = wk.gpw; p.waves = PWG_WAVES; p.items = wk.gps;
  p.items_hi = wk.gps < wk.gpw * PWG_WAVES ? wk.gps : wk.gpw * PWG_WAVES;
  p.items_lo = wk.gps - (wk.wps - 1) * wk.gpw * PWG_WAVES;
  p.nsplit_used = wk.wps * g.N; p.exact = 1;
  return true;
}

// The fp32-tensor kernels (tiled, persistent 16-channel, pointwise stream, producer / consumer), grouped launches included.
static int wgrad_tensor_plan(const cwf_wgrad_args& d, WgBf16Plan& p) {
  const int op = d.op, x3 = d.precision == CWF_BF16X3, groups = d.groups, N = d.N, Cin = d.Cin, Cout = d.Cout;
  const int Di = d.Di, Hi = d.Hi, Wi = d.Wi, Do = d.Do, Ho = d.Ho, Wo = d.Wo, x_ldc = d.x_ldc, dy_ldc = d.dy_ldc;
  // a grouped launch passes group 0's views through the plain fields
  const float* x = groups ? d.x_g[0] : d.x; const float* dy = groups ? d.dy_g[0] : d.dy; float* partial = groups ? d.partial_g[0] : d.partial;
  const float* in_scale = d.in_scale; const float* dy_scale = d.dy_scale;
  if (!x || !dy || !partial || N <= 0) return CWF_E_BADARG;
  // full-resolution 16-channel layers: persistent producer/consumer kernel (wgrad16_kernel), the only one that implements dy_scale
  const bool full16 = !groups && op == CWF_CONV3_S1 && Cin <= 16 && Cout == 16 && (dy_ldc & 3) == 0 && (((uintptr_t)dy) & 15) == 0 &&
                      (int64_t)Do * Ho * Wo >= 32768;
  if (dy_scale && !full16) return CWF_E_BADARG;
  if ((Cin & 3) || (x_ldc & 3) || ((uintptr_t)x & 15) || ((uintptr_t)partial & 15)) return CWF_E_ALIGN;
  if (in_scale && !d.in_shift) return CWF_E_BADARG;
  if (!(op == CWF_CONV3_S1 || op == CWF_CONV3_S2 || op == CWF_CONV1 || op == CWF_CONVT2)) return CWF_E_BADARG;
  const bool tapsplit = (op == CWF_CONV3_S1 || op == CWF_CONV3_S2);
  const int MTOT = (op == CWF_CONV3_S2) ? 4 : 16;
  const int nt_all = cdiv(Cout, 16);
  const int CG = tapsplit ? (nt_all == 1 ? 1 : 2) : (nt_all == 1 ? 1 : (nt_all == 2 ? 2 : 4));
  WgArgsB& a = p.a;
  int rc = cwf_build_geom(a.g, op, N, Di, Hi, Wi, Cin, x_ldc, Do, Ho, Wo, Cout, dy_ldc, MTOT);
  if (rc) return rc;
  const int nchunks = a.g.nchunks, ncls = a.g.ncls, ngroups = cdiv(a.g.ntiles, CG);
  int64_t blocks = 0;
  for (int c = 0; c < 8; ++c) { a.cls_slab_base[c] = (int)blocks; if (c < ncls) blocks += (int64_t)nchunks * ngroups * (a.g.cls_ntaps[c] + 1) * CG; }
  const int total = N * a.g.tiles_d * a.g.tiles_h * a.g.tiles_w;
  const int nblk = nchunks * ngroups * ncls;
  int want = 512 / nblk; if (want < 1) want = 1; if (want > total) want = total;
  const int tps = cdiv(total, want);
  const int wg_splits = cdiv(total, tps);
  // must agree with wgrad_mfma.hip's plan (the workspace was sized from it)
  if ((tapsplit ? wg_splits : wg_splits * 4) != cwf_wgrad_nsplit(op, N, Do, Ho, Wo, Cin, Cout) || blocks * 256 != cwf_wgrad_slab_floats(op, Cin, Cout))
    return CWF_E_BADARG;
  a.x = x; a.in_scale = in_scale; a.in_shift = d.in_shift; a.in_slope = d.in_slope; a.dy = dy; a.dy_ldc = dy_ldc; a.partial = partial;
  a.ngroups = ngroups; a.tiles_per_split = tps; a.total_tiles = total; a.slab_floats = blocks * 256;
  a.groups = groups; a.dy_scale = dy_scale;
  bool dy_al = (((uintptr_t)dy) & 15) == 0;
  for (int q = 0; q < 3; ++q) {
    a.x_g[q] = (groups && q < groups) ? d.x_g[q] : nullptr; a.dy_g[q] = (groups && q < groups) ? d.dy_g[q] : nullptr;
    a.partial_g[q] = (groups && q < groups) ? d.partial_g[q] : nullptr;
    if (groups && q < groups && (((uintptr_t)d.dy_g[q]) & 15)) dy_al = false;
  }
  p.CG = CG; p.slab = a.slab_floats; p.exact = 0;
  if (full16) {
    // one slab per workgroup (<= 256 <= generic nsplit)
    // (the stem layer -- 4 input channels -- is the LAST kernel of backward: nothing runs beside it, it takes every CU)
    int grid = Cin <= 4 ? 256 : SIDE_WGS; while (grid > 8 && grid > total) grid -= 8;      // multiple of 8 (XCD-aware tile map)
    p.id = x3 ? CWF_WGB_WGRAD16_X3 : CWF_WGB_WGRAD16; p.gx = grid; p.gy = 1; p.gz = 1; p.threads = 256 + 64 * W16_LW;
    p.lds = x3 ? W16Lds<true, false>::BYTES : W16Lds<false, false>::BYTES;
    wg_plan_strided(p, grid, total);
    p.nsplit_used = grid;
    return 0;
  }
  if (!groups && (op == CWF_CONV1 || op == CWF_CONVT2) && ((int64_t)Di * Hi * Wi & 3) == 0 && (op == CWF_CONV1 || (Wi & 3) == 0) &&
      (int64_t)Di * Hi * Wi * (x_ldc > 8 * dy_ldc ? x_ldc : 8 * dy_ldc) < (1ll << 31)) {
    // pointwise layers: stream kernel (fp32 MFMA straight from global memory, every operand read once), both precision modes
    const int nch = nchunks, ntl = a.g.ntiles;
    const int max_slabs = wg_splits * 4;                  // what the workspace was sized for
    bool ok = false;
    if (op == CWF_CONV1) {
      if (nch == 1 && ntl == 1) ok = pw_wgrad_plan<1, 1, 1>(p, CWF_WGB_PW_1_1_1, max_slabs);
      else if (nch == 2 && ntl == 1) ok = pw_wgrad_plan<2, 1, 1>(p, CWF_WGB_PW_2_1_1, max_slabs);
      else if (nch == 4 && ntl == 2) ok = pw_wgrad_plan<4, 2, 1>(p, CWF_WGB_PW_4_2_1, max_slabs);
      else if (nch == 8 && ntl == 4) ok = pw_wgrad_plan<8, 4, 1>(p, CWF_WGB_PW_8_4_1, max_slabs);
    } else {
      if (nch == 1 && ntl == 1) ok = pw_wgrad_plan<1, 1, 8>(p, CWF_WGB_PW_1_1_8, max_slabs);
      else if (nch == 2 && ntl == 2) ok = pw_wgrad_plan<2, 2, 8>(p, CWF_WGB_PW_2_2_8, max_slabs);
    }
    if (ok) return 0;
  }
  if (!x3 && op == CWF_CONV3_S1 && CG <= 2 && a.g.TD == 4 && a.g.TH == 4 && a.g.ID == 6 && a.g.IH == 6 && a.g.IW == 18 && (Cout & 3) == 0 &&
      (dy_ldc & 3) == 0 && dy_al) {
    // producer / consumer kernel: ~256 eight-wave workgroups in all (one per CU), each a contiguous tile range of one (chunk, group)
    int want1 = SIDE_WGS / nblk; if (want1 < 1) want1 = 1; if (want1 > total) want1 = total;
    const int tps1 = cdiv(total, want1), splits1 = cdiv(total, tps1);
    if (splits1 <= wg_splits) {                          // (the workspace was sized for wg_splits slabs)
      a.tiles_per_split = tps1;
      p.id = CG == 1 ? CWF_WGB_S1_1 : CWF_WGB_S1_2; p.gx = splits1; p.gy = nchunks * ngroups; p.gz = groups ? groups : 1;
      p.threads = 256 + 64 * WS1_LW; p.lds = CG == 1 ? Ws1Lds<1, false>::BYTES : Ws1Lds<2, false>::BYTES;
      wg_plan_ranges(p, splits1, tps1, total);
      p.nsplit_used = splits1;
      return 0;
    }
  }
  const size_t ximg = (size_t)a.g.ID * a.g.IH * wg_x_pitch(a.g.IW, a.g.is) * 16;
  const size_t dimg = (size_t)a.g.TD * a.g.TH * wg_dy_pitch(CG * 16) * CG * 16 + (size_t)(a.g.TD * a.g.TH / 2 + 1) * wg_dy_skew(CG * 16);
  p.lds = (ximg + dimg) * sizeof(unsigned short) * (x3 ? 2 : 1);
  if (p.lds > 160 * 1024) return CWF_E_TOOLARGE;
  if (tapsplit) p.id = (CG == 1 ? CWF_WGB_TILED_7_1 : CWF_WGB_TILED_7_2) + x3;
  else p.id = (CG == 1 ? CWF_WGB_TILED_2_1 : (CG == 2 ? CWF_WGB_TILED_2_2 : CWF_WGB_TILED_2_4)) + x3;
  p.gx = wg_splits; p.gy = nchunks * ngroups; p.gz = groups ? groups : ncls;     // grid z: group (grouped launches are single-class) or parity class
  p.threads = 256;
  wg_plan_ranges(p, wg_splits, tps, total);
  p.nsplit_used = tapsplit ? wg_splits : wg_splits * 4;  // (the 1-tap kernel: every wave writes its own slab)
  return 0;
}

// The one place that chooses a bf16-form weight-gradient slab kernel (include/cwf_hip.h, struct cwf_wgrad_args).
static int wgrad_bf16_plan(const cwf_wgrad_args& d, WgBf16Plan& p) {
  if (d.precision != CWF_FP32 && d.precision != CWF_BF16X3 && d.precision != CWF_BF16) return CWF_E_BADARG;
  if (d.xa16 || d.dy16) {                                  // bf16 operand images (x, dy and x's prologue are not read)
    if (!d.xa16 || !d.dy16 || d.precision != CWF_BF16 || d.op != CWF_CONV3_S1 || d.groups || d.dy_scale) return CWF_E_BADARG;
    if (d.Cin == 16 && d.Cout == 16 && (int64_t)d.Do * d.Ho * d.Wo >= 32768) return wgrad16d_plan(d, p);
    return wgrad_s1d_plan(d, p);
  }
  if (d.groups) {
    if (d.groups < 2 || d.groups > 3 || d.op != CWF_CONV3_S1 || d.precision == CWF_FP32 || d.in_scale || d.dy_scale) return CWF_E_BADARG;
    for (int q = 0; q < d.groups; ++q)
      if (!d.x_g[q] || !d.dy_g[q] || !d.partial_g[q] || ((uintptr_t)d.x_g[q] & 15) || ((uintptr_t)d.partial_g[q] & 15)) return CWF_E_ALIGN;
    return wgrad_tensor_plan(d, p);
  }
  if (d.precision == CWF_FP32) return CWF_E_BADARG;       // (cwf_wgrad: wgrad_fp32_launch, wgrad_mfma.hip)
  return wgrad_tensor_plan(d, p);
}

// Route of the single-bf16 stride-2 launches behind TILED_7_1 / TILED_7_2 (include/cwf_hip.h): 1 = wgrad_s2_kernel, 0 = the tiled kernel.
static int g_wgrad_s2 = 1;
static long long g_wgrad_s2_launches = 0;
extern "C" int cwf_debug_wgrad_s2(int v) { const int old = g_wgrad_s2; g_wgrad_s2 = v; return old; }
extern "C" long long cwf_debug_wgrad_s2_launches() { return g_wgrad_s2_launches; }

// wgrad_s2_kernel takes a tiled plan when the geometry is the one it has compiled in and dy needs no scalar path
static bool wgrad_s2_takes(const WgBf16Plan& p) {
  if (p.id != CWF_WGB_TILED_7_1 && p.id != CWF_WGB_TILED_7_2) return false;
  const WgArgsB& a = p.a; const ConvGeom& g = a.g;
  if (a.groups || p.threads != 256 || g.ncls != 1 || g.is != 2 || g.os != 1 || g.TD != 2 || g.TH != 2 || g.ID != 5 || g.IH != 5 || g.IW != 33 ||
      g.cls_ntaps[0] != 27 || g.tiles_d != cdiv(g.cls_dims[0][0], 2) || g.tiles_h != cdiv(g.cls_dims[0][1], 2) || g.tiles_w != cdiv(g.cls_dims[0][2], 16))
    return false;
  for (int t = 0; t < 27; ++t) if (g.tapofs[t] != ((t / 9) * 5 + (t / 3) % 3) * 33 + t % 3) return false;
  if ((a.dy_ldc & 3) || ((uintptr_t)a.dy & 15) || g.Cout > a.dy_ldc || g.y_ldc != a.dy_ldc) return false;
  return (int64_t)6 * g.Hi * g.Wi * g.x_ldc < (1ll << 31);   // (a thread's slot offsets inside a halo are 32-bit)
}

template <int NTW>
static void wgrad_s2_launch(const WgBf16Plan& p, dim3 grid, hipStream_t st) {
  CWF_MAX_LDS_ONCE((&wgrad_s2_kernel<NTW>));
  hipLaunchKernelGGL((wgrad_s2_kernel<NTW>), grid, dim3(256), WgS2Lds<NTW>::BYTES, st, p.a);
}

static int wgrad_bf16_launch(const WgBf16Plan& p, int* nsplit_used, hipStream_t st) {
  const dim3 grid(p.gx, p.gy, p.gz), block(p.threads);
  if (g_wgrad_s2 && wgrad_s2_takes(p)) {
    if (p.id == CWF_WGB_TILED_7_1) wgrad_s2_launch<1>(p, grid, st);
    else wgrad_s2_launch<2>(p, grid, st);
    ++g_wgrad_s2_launches;
    CWF_LAUNCH_CHECK();
    if (nsplit_used) *nsplit_used = p.nsplit_used;
    return 0;
  }
#define CWF_WGK(id_, ...) case id_: CWF_MAX_LDS_ONCE((&__VA_ARGS__)); hipLaunchKernelGGL((__VA_ARGS__), grid, block, p.lds, st, p.a); break
#define CWF_WGP(id_, ...) case id_: hipLaunchKernelGGL((__VA_ARGS__), grid, block, 0, st, p.a, p.wk, p.CG); break
  switch (p.id) {
    case CWF_WGB_WGRAD16: CWF_MAX_LDS_ONCE((&wgrad16_kernel<false>)); hipLaunchKernelGGL((wgrad16_kernel<false>), grid, block, p.lds, st, p.a, p.a.total_tiles); break;
    case CWF_WGB_WGRAD16_X3: CWF_MAX_LDS_ONCE((&wgrad16_kernel<true>)); hipLaunchKernelGGL((wgrad16_kernel<true>), grid, block, p.lds, st, p.a, p.a.total_tiles); break;
    CWF_WGP(CWF_WGB_PW_1_1_1, pw_wgrad_kernel<1, 1, 1>);
    CWF_WGP(CWF_WGB_PW_2_1_1, pw_wgrad_kernel<2, 1, 1>);
    CWF_WGP(CWF_WGB_PW_4_2_1, pw_wgrad_kernel<4, 2, 1>);
    CWF_WGP(CWF_WGB_PW_8_4_1, pw_wgrad_kernel<8, 4, 1>);
    CWF_WGP(CWF_WGB_PW_1_1_8, pw_wgrad_kernel<1, 1, 8>);
    CWF_WGP(CWF_WGB_PW_2_2_8, pw_wgrad_kernel<2, 2, 8>);
    case CWF_WGB_S1_1: case CWF_WGB_S1_2:
      CWF_MAX_LDS_ONCE((&wgrad_s1_kernel<1>));
      CWF_MAX_LDS_ONCE((&wgrad_s1_kernel<2>));
      if (p.id == CWF_WGB_S1_1) hipLaunchKernelGGL((wgrad_s1_kernel<1>), grid, block, p.lds, st, p.a);
      else hipLaunchKernelGGL((wgrad_s1_kernel<2>), grid, block, p.lds, st, p.a);
      break;
    CWF_WGK(CWF_WGB_TILED_7_1, wgrad_bf16_kernel<7, 1, true, false>);
    CWF_WGK(CWF_WGB_TILED_7_1_X3, wgrad_bf16_kernel<7, 1, true, true>);
    CWF_WGK(CWF_WGB_TILED_7_2, wgrad_bf16_kernel<7, 2, true, false>);
    CWF_WGK(CWF_WGB_TILED_7_2_X3, wgrad_bf16_kernel<7, 2, true, true>);
    CWF_WGK(CWF_WGB_TILED_2_1, wgrad_bf16_kernel<2, 1, false, false>);
    CWF_WGK(CWF_WGB_TILED_2_1_X3, wgrad_bf16_kernel<2, 1, false, true>);
    CWF_WGK(CWF_WGB_TILED_2_2, wgrad_bf16_kernel<2, 2, false, false>);
    CWF_WGK(CWF_WGB_TILED_2_2_X3, wgrad_bf16_kernel<2, 2, false, true>);
    CWF_WGK(CWF_WGB_TILED_2_4, wgrad_bf16_kernel<2, 4, false, false>);
    CWF_WGK(CWF_WGB_TILED_2_4_X3, wgrad_bf16_kernel<2, 4, false, true>);
    case CWF_WGB_WGRAD16D:
      CWF_MAX_LDS_ONCE((&wgrad16d_kernel));
      hipLaunchKernelGGL(wgrad16d_kernel, grid, block, p.lds, st, static_cast<const W16dArgs&>(p.ad));
      break;
    case CWF_WGB_S1D: CWF_MAX_LDS_ONCE((&wgrad_s1d_kernel)); hipLaunchKernelGGL(wgrad_s1d_kernel, grid, block, p.lds, st, p.ad); break;
    default: return CWF_E_BADARG;
  }
#undef CWF_WGP
#undef CWF_WGK
  CWF_LAUNCH_CHECK();
  if (nsplit_used) *nsplit_used = p.nsplit_used;
  return 0;
}

extern "C" int cwf_wgrad(const struct cwf_wgrad_args* args, int* nsplit_used, void* stream) {
  if (!args) return CWF_E_BADARG;
  const cwf_wgrad_args& d = *args;
  if (d.precision != CWF_FP32 && d.precision != CWF_BF16X3 && d.precision != CWF_BF16) return CWF_E_BADARG;
  hipStream_t st = cwf_stream(stream);
  if (d.precision == CWF_FP32 && !d.xa16 && !d.dy16 && !d.groups) return d.dy_scale ? CWF_E_BADARG : wgrad_fp32_launch(d, nsplit_used, st);
  WgBf16Plan p;
  if (const int rc = wgrad_bf16_plan(d, p)) return rc;
  return wgrad_bf16_launch(p, nsplit_used, st);
}

extern "C" int cwf_debug_wgrad_bf16_plan(const struct cwf_wgrad_args* args, int64_t* out) {
  if (!args || !out) return CWF_E_BADARG;
  WgBf16Plan p;
  if (const int rc = wgrad_bf16_plan(*args, p)) return rc;
  const bool pw = p.walk == CWF_WGB_WALK_PW;
  const int64_t v[CWF_WGB_PLAN_FIELDS] = {p.id, p.gx, p.gy, p.gz, p.threads, p.walk, p.walk_step, pw ? p.wk.wps : 0, p.waves, p.items,
                                          p.slab, p.nsplit_used, p.exact, p.items_lo, p.items_hi};
  for (int i = 0; i < CWF_WGB_PLAN_FIELDS; ++i) out[i] = v[i];
  return 0;
}

extern "C" const char* cwf_debug_wgrad_bf16_name(int instance) {
  static const char* const names[CWF_WGB_COUNT] = {
    "wgrad16", "wgrad16_x3", "pw_wgrad<1,1,1>", "pw_wgrad<2,1,1>", "pw_wgrad<4,2,1>", "pw_wgrad<8,4,1>", "pw_wgrad<1,1,8>", "pw_wgrad<2,2,8>",
    "wgrad_s1<1>", "wgrad_s1<2>", "wgrad_bf16<7,1,ts>", "wgrad_bf16<7,1,ts,x3>", "wgrad_bf16<7,2,ts>", "wgrad_bf16<7,2,ts,x3>",
    "wgrad_bf16<2,1>", "wgrad_bf16<2,1,x3>", "wgrad_bf16<2,2>", "wgrad_bf16<2,2,x3>", "wgrad_bf16<2,4>", "wgrad_bf16<2,4,x3>",
    "wgrad16d", "wgrad_s1d"};
  return (instance >= 0 && instance < CWF_WGB_COUNT) ? names[instance] : nullptr;
}
