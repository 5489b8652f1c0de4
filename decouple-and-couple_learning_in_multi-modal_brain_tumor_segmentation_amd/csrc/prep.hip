// N3 -- training-batch preparation on the device (utils/data.py prepare_batch / DeviceBraTS).  One launch per (up to) eight samples
// turns source volumes into (x, target, edge):
//   source coordinate  s_i = o_i + (flip_i ? C_i-1-p_i : p_i); s_i >= S_i is outside the volume (image 0, label 0)
//                      = utils.data.crop_pad followed by torch.flip of the crop
//   x                  copied bit for bit, or fadd_rn(fmul_rn(v, scale_c), shift_c) with intensity on (padded voxels: 0 * scale + shift)
//   target             the label with 4 -> 3, as int64
//   edge               utils.synthetic.edge_codes of the cropped, flipped target (max_pool3d footprint: out-of-crop neighbours ignored)
//
// Edge codes, separably: every voxel carries six bits, any_k (bits 0-2) and all_k (bits 3-5) of (label == k), k = 1, 2, 3.  Three 1-D
// passes over the 3-box take OR of the any bits and AND of the all bits, out-of-crop voxels being the identity of both (0x38); then
// band_k = any_k & ~all_k = dilate(R_k) & ~erode(R_k) and the code is membership-coded as edge_codes does.  The bits of four
// consecutive voxels sit in one 32-bit word (one byte each), so every pass step is one OR and one AND per four voxels.
//
// Tile: 4 x 16 x 64 output voxels per 256-thread workgroup; each thread owns four quads (4 voxels along the contiguous axis, one
// quad per axis-0 slice).  LDS holds the label-bit halo [6][18][68 B], the axis-2 pass [6][18][16 words] and the axis-1 pass
// [6][16][16 words] (20.4 KiB).  The image is read with dword loads -- crop origins are arbitrary, so source rows have no 16-B
// alignment, and a flipped contiguous axis is read in descending order by the same loads -- and written with one 16-B store per
// quad and channel; target and edge with two 16-B stores per quad (two int64 voxels each).  Crops whose rows are not a multiple of
// four voxels, or outputs without 16-B alignment, take the same kernel with per-voxel stores.
//
// cwf_prepare_batch_affine: the same outputs from a rotated and zoomed crop (trilinear image, nearest label), a kernel of its own
// further down on an 8 x 8 x 32 tile.  cwf_prepare_batch_elastic: that kernel's second instantiation, which adds a cubic B-spline
// displacement to every source coordinate.
//
// What the kernels share is written once: the tile description (PrepTile), the three passes with the target / edge store
// (prep_tail), the image-quad store (prep_store_quad) and, on the host, the checks and the launch loop of all three entries
// (prep_launch).  A kernel keeps its own halo fill and image pass.  The samples travel as the public structs of include/cwf_hip.h.
//
// cwf_normalize_nonzero: per-channel z-score over the voxels whose four-channel sum ((x0 + x1) + x2) + x3 (float32) is > 0, float64
// two-pass statistics (partials per workgroup, reduced in a fixed order by one thread: the result does not depend on scheduling).
// This file is compiled with -ffp-contract=off.
#include "common.h"

#define PREP_MAXS 8                         // samples per launch

// the T0 x T1 x T2 output voxels of a 256-thread workgroup and what follows from them
template <int T0_, int T1_, int T2_>
struct PrepTile {
  static constexpr int T0 = T0_, T1 = T1_, T2 = T2_;
  static constexpr int Q2 = T2 / 4;                           // quads per tile row
  static constexpr int H0 = T0 + 2, H1 = T1 + 2, H2 = T2 + 2; // the tile with its one-voxel halo
  static constexpr int ROW = (H2 + 3) / 4 * 4;                // halo row bytes (H2 used, padded to whole words)
  static constexpr int QUADS = T0 * T1 * Q2 / 256;            // quads per thread
  static_assert(T2 % 4 == 0 && QUADS * 256 == T0 * T1 * Q2, "whole quads, the same number for every thread");
};
typedef PrepTile<4, 16, 64> PlainTile;      // 68-byte halo row, one quad per thread and axis-0 slice
typedef PrepTile<8, 8, 32> AffTile;         // 36-byte halo row (the choice: further down)

template <class Sample>
struct PrepArgs {
  Sample s[PREP_MAXS];
  float* x;
  int64_t* target;
  int64_t* edge;
  int64_t x_bs, t_bs, e_bs;                 // sample strides (elements)
  int C0, C1, C2, vec;
};

__device__ __forceinline__ uint32_t prep_or_and(uint32_t a, uint32_t b, uint32_t c) {
  return ((a | b | c) & 0x07070707u) | ((a & b & c) & 0x38383838u);
}

// label bits of a source label: {1, 2, 3|4} -> any and all bit of that region; anything else (0) -> none
__device__ __forceinline__ uint32_t prep_bits(uint32_t l) {
  return l == 1 ? 0x09u : l == 2 ? 0x12u : (l == 3 || l == 4) ? 0x24u : 0u;
}

__device__ __forceinline__ int64_t prep_label(uint32_t bits) {
  return (bits & 1u) ? 1 : (bits & 2u) ? 2 : (bits & 4u) ? 3 : 0;
}

__device__ __forceinline__ int64_t prep_code(uint32_t band) {
  // band = b1 | b2 << 1 | b4 << 2  ->  edge_codes: 1, 2, 4 alone; 6 = 1&2, 7 = 1&4, 8 = 2&4, 5 = all three
  return (int64_t)((0x58746210u >> (4u * band)) & 0xFu);
}

// one channel's quad of image voxels at d, the quad starting at output index p2 of a row of C2 voxels
__device__ __forceinline__ void prep_store_quad(float* d, const float (&v)[4], int vec, int p2, int C2) {
  if (vec) {
    f32x4 o = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(d) = o;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (p2 + e < C2) d[e] = v[e];
  }
}

// The part every kernel ends with, entered after the barrier that completes the label-bit halo H of the tile at (b0, b1, b2): the
// axis-2 and axis-1 passes through P1 and P2, the axis-0 pass in registers, and target and edge of the tile's voxels.
template <class T, class Args>
__device__ __forceinline__ void prep_tail(uint8_t (&H)[T::H0][T::H1][T::ROW], uint32_t (&P1)[T::H0][T::H1][T::Q2],
                                                 uint32_t (&P2)[T::H0][T::T1][T::Q2], const Args& a, int b0, int b1, int b2) {
  const int C0 = a.C0, C1 = a.C1, C2 = a.C2;
  const int tid = threadIdx.x;
  // axis-2 pass: [H0][H1][Q2 quads]
  for (int i = tid; i < T::H0 * T::H1 * T::Q2; i += 256) {
    const int w = i % T::Q2, h1 = (i / T::Q2) % T::H1, h0 = i / (T::Q2 * T::H1);
    const uint32_t* row = reinterpret_cast<const uint32_t*>(&H[h0][h1][0]);
    const uint32_t w0 = row[w], w1 = row[w + 1];
    P1[h0][h1][w] = prep_or_and(w0, (w0 >> 8) | (w1 << 24), (w0 >> 16) | (w1 << 16));
  }
  __syncthreads();
  // axis-1 pass: [H0][T1][Q2]
  for (int i = tid; i < T::H0 * T::T1 * T::Q2; i += 256) {
    const int w = i % T::Q2, j = (i / T::Q2) % T::T1, h0 = i / (T::Q2 * T::T1);
    P2[h0][j][w] = prep_or_and(P1[h0][j][w], P1[h0][j + 1][w], P1[h0][j + 2][w]);
  }
  __syncthreads();

  // axis-0 pass in registers, target and edge codes
  int64_t* ts = a.target + (int64_t)blockIdx.y * a.t_bs;
  int64_t* es = a.edge + (int64_t)blockIdx.y * a.e_bs;
#pragma unroll 1
  for (int k = 0; k < T::QUADS; ++k) {
    const int q = tid + 256 * k;
    const int w = q % T::Q2, j = (q / T::Q2) % T::T1, i = q / (T::Q2 * T::T1);
    const int p0 = b0 + i, p1 = b1 + j, p2 = b2 + 4 * w;
    if (p0 >= C0 || p1 >= C1 || p2 >= C2) continue;
    const uint32_t r = prep_or_and(P2[i][j][w], P2[i + 1][j][w], P2[i + 2][j][w]);
    const uint32_t band = (r & 0x07070707u) & ~((r >> 3) & 0x07070707u);
    const uint32_t* row = reinterpret_cast<const uint32_t*>(&H[i + 1][j + 1][0]);
    const uint32_t centre = (row[w] >> 8) | (row[w + 1] << 24);
    int64_t tl[4], ec[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      tl[e] = prep_label((centre >> (8 * e)) & 0xFFu);
      ec[e] = prep_code((band >> (8 * e)) & 0xFFu);
    }
    const int64_t dst = ((int64_t)p0 * C1 + p1) * C2 + p2;
    if (a.vec) {
      typedef long long i64x2 __attribute__((ext_vector_type(2)));
      i64x2* tp = reinterpret_cast<i64x2*>(ts + dst);
      i64x2* ep = reinterpret_cast<i64x2*>(es + dst);
      tp[0] = i64x2{tl[0], tl[1]};
      tp[1] = i64x2{tl[2], tl[3]};
      ep[0] = i64x2{ec[0], ec[1]};
      ep[1] = i64x2{ec[2], ec[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p2 + e < C2) {
          ts[dst + e] = tl[e];
          es[dst + e] = ec[e];
        }
    }
  }
}

__global__ __launch_bounds__(256) void prep_batch_kernel(const PrepArgs<cwf_prep_sample> a) {
  typedef PlainTile T;
  __shared__ __attribute__((aligned(16))) uint8_t H[T::H0][T::H1][T::ROW];
  __shared__ uint32_t P1[T::H0][T::H1][T::Q2];
  __shared__ uint32_t P2[T::H0][T::T1][T::Q2];
  const cwf_prep_sample& S = a.s[blockIdx.y];
  const int C0 = a.C0, C1 = a.C1, C2 = a.C2;
  const int n2 = (C2 + T::T2 - 1) / T::T2, n1 = (C1 + T::T1 - 1) / T::T1;
  const int t = blockIdx.x;
  const int b2 = (t % n2) * T::T2, b1 = ((t / n2) % n1) * T::T1, b0 = (t / (n2 * n1)) * T::T0;
  const int f0 = S.flip & 1, f1 = (S.flip >> 1) & 1, f2 = (S.flip >> 2) & 1;
  const int64_t plane = (int64_t)S.S1 * S.S2, V = (int64_t)S.S0 * plane;
  const int tid = threadIdx.x;

  // 1. label bits of the halo tile
  for (int i = tid; i < T::H0 * T::H1 * T::H2; i += 256) {
    const int h2 = i % T::H2, h1 = (i / T::H2) % T::H1, h0 = i / (T::H2 * T::H1);
    const int p0 = b0 + h0 - 1, p1 = b1 + h1 - 1, p2 = b2 + h2 - 1;
    uint32_t v = 0x38u;                                       // out of the crop: identity of OR and AND
    if (p0 >= 0 && p0 < C0 && p1 >= 0 && p1 < C1 && p2 >= 0 && p2 < C2) {
      const int s0 = S.o0 + (f0 ? C0 - 1 - p0 : p0), s1 = S.o1 + (f1 ? C1 - 1 - p1 : p1), s2 = S.o2 + (f2 ? C2 - 1 - p2 : p2);
      v = (s0 < S.S0 && s1 < S.S1 && s2 < S.S2) ? prep_bits(S.label[s0 * plane + (int64_t)s1 * S.S2 + s2]) : 0u;
    }
    H[h0][h1][h2] = (uint8_t)v;
  }

  // 2. image: independent of the label tile, issued before the first barrier's wait
  const bool inten = S.intensity != 0;
  const int64_t V_out = (int64_t)C0 * C1 * C2;
  float* xs = a.x + (int64_t)blockIdx.y * a.x_bs;
#pragma unroll 1
  for (int k = 0; k < T::QUADS; ++k) {
    const int q = tid + 256 * k;
    const int w = q % T::Q2, j = (q / T::Q2) % T::T1, i = q / (T::Q2 * T::T1);
    const int p0 = b0 + i, p1 = b1 + j, p2 = b2 + 4 * w;
    if (p0 >= C0 || p1 >= C1 || p2 >= C2) continue;
    const int s0 = S.o0 + (f0 ? C0 - 1 - p0 : p0), s1 = S.o1 + (f1 ? C1 - 1 - p1 : p1);
    const bool row_in = s0 < S.S0 && s1 < S.S1;
    const int64_t src_row = s0 * plane + (int64_t)s1 * S.S2;
    const int64_t dst = ((int64_t)p0 * C1 + p1) * C2 + p2;
    int s2[4];
    bool in[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s2[e] = S.o2 + (f2 ? C2 - 1 - (p2 + e) : p2 + e);
      in[e] = row_in && p2 + e < C2 && s2[e] < S.S2;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* src = S.image + c * V + src_row;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = in[e] ? src[s2[e]] : 0.f;
        if (inten) v[e] = __fadd_rn(__fmul_rn(v[e], S.scale[c]), S.shift[c]);
      }
      prep_store_quad(xs + c * V_out + dst, v, a.vec, p2, C2);
    }
  }
  __syncthreads();
  prep_tail<T>(H, P1, P2, a, b0, b1, b2);
}

// ------------------------------------------------------------------------------------------------ rotated / zoomed crops
// cwf_prepare_batch_affine: the same outputs from a resampled crop (statement: include/cwf_hip.h, utils.data._prepare_one_cpu).  The
// halo tile is filled through the nearest-neighbour map, after which the passes are those of prep_batch_kernel on a smaller tile:
// 8 x 8 x 32 output voxels per 256-thread workgroup (two quads per thread).  Under a rotation a tile reads a box of the source that is
// as large along every axis as the tile's longest side, so the tile is kept near-cubic: 8 x 8 x 32 touches about 43 KB of image
// (four channels) where 4 x 16 x 64 would touch several times that, and its taps are served by the CU's vector cache and L2.  LDS:
// halo [10][10][36 B], passes [10][10][8] and [10][8][8] words (9.4 KiB).
#define AFF_QMAX 1073741824.f               // |q| at and beyond 2^30 (and NaN): the voxel lies outside every volume

// the elastic entry's sample on the device: G* zeroed when disp == nullptr (nothing is added); k[d] = float(G_d - 3) / float(C_d - 1),
// divided on the host
struct PrepElaSample : cwf_prep_elastic_sample {
  float k[3];
};
static_assert(sizeof(PrepArgs<PrepElaSample>) <= 4096, "the samples travel by value in the kernel-argument block");

// crop-local source coordinate of the (already flipped) output voxel (p0, p1, p2); false when it is not representable
__device__ __forceinline__ bool aff_coord(const float (&m)[9], int p0, int p1, int p2, float c0, float c1, float c2, float q[3]) {
  const float u0 = __fsub_rn((float)p0, c0), u1 = __fsub_rn((float)p1, c1), u2 = __fsub_rn((float)p2, c2);
  const float c[3] = {c0, c1, c2};
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    q[d] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[3 * d], u0), __fmul_rn(m[3 * d + 1], u1)), __fmul_rn(m[3 * d + 2], u2)), c[d]);
    ok = ok && fabsf(q[d]) < AFF_QMAX;
  }
  return ok;
}

__device__ __forceinline__ float aff_lerp(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(f, __fsub_rn(b, a))); }

// Elastic deformation (statement: include/cwf_hip.h).  The spline is separable, so a workgroup evaluates the four weights and the four
// clamped control indices (times the grid stride of their axis) of its 10 + 10 + 34 halo coordinates once; a voxel then needs three
// table rows and 64 control points.  The sample's whole grid (at most 8^3 points, the three components of a point side by side) is
// staged in LDS, so no control index ever forms a global address: 8 KiB for the grid and 1.7 KiB for the tables.
#define ELA_GMAX 8
#define ELA_ROWS (AffTile::H0 + AffTile::H1 + AffTile::H2)
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct ElaTables {
  f32x4 cg[ELA_GMAX * ELA_GMAX * ELA_GMAX];   // control point [i0][i1][i2] -> (disp[0], disp[1], disp[2], 0)
  f32x4 w[ELA_ROWS];                          // rows 0..9 axis 0, 10..19 axis 1, 20..53 axis 2 (halo coordinate h = p - b + 1)
  i32x4 ix[ELA_ROWS];
};

// ((w0*a + w1*b) + w2*c) + w3*d
__device__ __forceinline__ float ela_sum4(f32x4 w, float a, float b, float c, float d) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w[0], a), __fmul_rn(w[1], b)), __fmul_rn(w[2], c)), __fmul_rn(w[3], d));
}

// weights and control indices of the output index p (not yet flipped) along an axis of C voxels and G control points
__device__ __forceinline__ void ela_axis(int p, int C, bool flip, int G, float k, int stride, f32x4& w, i32x4& ix) {
  w = f32x4{0.f, 0.f, 0.f, 0.f};
  ix = i32x4{0, 0, 0, 0};
  if (p < 0 || p >= C) return;                                // a halo coordinate outside the crop: never looked up
  const float g = __fadd_rn(__fmul_rn((float)(flip ? C - 1 - p : p), k), 1.f);
  const float fl = floorf(g);
  const float t = __fsub_rn(g, fl), s = __fsub_rn(1.f, t), h = 0.16666667163372040f;
  w[0] = __fmul_rn(__fmul_rn(__fmul_rn(s, s), s), h);
  w[1] = __fmul_rn(__fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(3.f, t), 6.f), t), t), 4.f), h);
  w[2] = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(-3.f, t), 3.f), t), 3.f), t), 1.f), h);
  w[3] = __fmul_rn(__fmul_rn(__fmul_rn(t, t), t), h);
  const int i = (int)fl;                                      // 1 <= g <= G - 2 + one rounding: i is in [1, G - 2]
#pragma unroll
  for (int j = 0; j < 4; ++j) ix[j] = min(max(i - 1 + j, 0), G - 1) * stride;
}

__device__ __forceinline__ void ela_setup(const PrepElaSample& S, ElaTables& T, int b0, int b1, int b2, int C0, int C1, int C2, int tid) {
  const int n = S.G0 * S.G1 * S.G2;                           // <= 512 (checked on the host)
  for (int i = tid; i < n; i += 256) T.cg[i] = f32x4{S.disp[i], S.disp[n + i], S.disp[2 * n + i], 0.f};
  if (tid >= ELA_ROWS) return;
  f32x4 w;
  i32x4 ix;
  if (tid < AffTile::H0)
    ela_axis(b0 + tid - 1, C0, S.flip & 1, S.G0, S.k[0], S.G1 * S.G2, w, ix);
  else if (tid < AffTile::H0 + AffTile::H1)
    ela_axis(b1 + (tid - AffTile::H0) - 1, C1, (S.flip >> 1) & 1, S.G1, S.k[1], S.G2, w, ix);
  else
    ela_axis(b2 + (tid - AffTile::H0 - AffTile::H1) - 1, C2, (S.flip >> 2) & 1, S.G2, S.k[2], 1, w, ix);
  T.w[tid] = w;
  T.ix[tid] = ix;
}

// q += D at the halo coordinate (h0, h1, h2) of the tile, then the |q| < 2^30 test on the result.  The outer sum runs as a loop that
// is not unrolled (a running ((a + b) + c) + d is the same association): unrolled, the 64 control points of each of a thread's four
// voxels are all fetched ahead and the kernel needs several times the registers.
__device__ __forceinline__ bool ela_displace(const ElaTables& T, int h0, int h1, int h2, float q[3]) {
  const f32x4 w1 = T.w[AffTile::H0 + h1], w2 = T.w[AffTile::H0 + AffTile::H1 + h2];
  const i32x4 i1 = T.ix[AffTile::H0 + h1], i2 = T.ix[AffTile::H0 + AffTile::H1 + h2];
  const float* w0 = reinterpret_cast<const float*>(&T.w[h0]);
  const int* i0 = reinterpret_cast<const int*>(&T.ix[h0]);
  float D[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
  for (int j0 = 0; j0 < 4; ++j0) {
    float r1[3][4];
#pragma unroll
    for (int j1 = 0; j1 < 4; ++j1) {
      const int row = i0[j0] + i1[j1];
      const f32x4 a = T.cg[row + i2[0]], b = T.cg[row + i2[1]], c = T.cg[row + i2[2]], d = T.cg[row + i2[3]];
#pragma unroll
      for (int e = 0; e < 3; ++e) r1[e][j1] = ela_sum4(w2, a[e], b[e], c[e], d[e]);
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const float v = __fmul_rn(w0[j0], ela_sum4(w1, r1[e][0], r1[e][1], r1[e][2], r1[e][3]));
      D[e] = j0 == 0 ? v : __fadd_rn(D[e], v);
    }
  }
  bool ok = true;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    q[e] = __fadd_rn(q[e], D[e]);
    ok = ok && fabsf(q[e]) < AFF_QMAX;
  }
  return ok;
}

// the source coordinate of the (unflipped) output voxel (p0, p1, p2) = halo coordinate (h0, h1, h2): the one place both the label
// pass and the image pass take it from
template <bool DISP, class Sample>
__device__ __forceinline__ bool res_coord(const Sample& S, const ElaTables* T, bool disp, int p0, int p1, int p2, int h0, int h1, int h2,
                                          int C0, int C1, int C2, float c0, float c1, float c2, float q[3]) {
  const bool ok = aff_coord(S.m, (S.flip & 1) ? C0 - 1 - p0 : p0, (S.flip & 2) ? C1 - 1 - p1 : p1, (S.flip & 4) ? C2 - 1 - p2 : p2, c0, c1, c2, q);
  if constexpr (DISP) {
    if (disp) return ela_displace(*T, h0, h1, h2, q);          // the test is on the final q alone
  }
  return ok;
}

template <class Sample>
__global__ __launch_bounds__(256) void prep_affine_kernel(const PrepArgs<Sample> a) {
  constexpr bool DISP = std::is_same<Sample, PrepElaSample>::value;
  __shared__ __attribute__((aligned(16))) uint8_t H[AffTile::H0][AffTile::H1][AffTile::ROW];
  __shared__ uint32_t P1[AffTile::H0][AffTile::H1][AffTile::Q2];
  __shared__ uint32_t P2[AffTile::H0][AffTile::T1][AffTile::Q2];
  const Sample& S = a.s[blockIdx.y];
  const int C0 = a.C0, C1 = a.C1, C2 = a.C2;
  const int n2 = (C2 + AffTile::T2 - 1) / AffTile::T2, n1 = (C1 + AffTile::T1 - 1) / AffTile::T1;
  const int t = blockIdx.x;
  const int b2 = (t % n2) * AffTile::T2, b1 = ((t / n2) % n1) * AffTile::T1, b0 = (t / (n2 * n1)) * AffTile::T0;
  const float c0 = 0.5f * (float)(C0 - 1), c1 = 0.5f * (float)(C1 - 1), c2 = 0.5f * (float)(C2 - 1);
  const int64_t S0 = S.S0, S1 = S.S1, S2 = S.S2, plane = S1 * S2, V = S0 * plane;
  const int tid = threadIdx.x;
  const ElaTables* T = nullptr;
  bool disp = false;
  if constexpr (DISP) {
    __shared__ ElaTables tables;
    T = &tables;
    disp = S.disp != nullptr;                                 // uniform over the workgroup
    if (disp) ela_setup(S, tables, b0, b1, b2, C0, C1, C2, tid);
    __syncthreads();
  }

  // 1. label bits of the halo tile, through the nearest-neighbour map
  for (int i = tid; i < AffTile::H0 * AffTile::H1 * AffTile::H2; i += 256) {
    const int h2 = i % AffTile::H2, h1 = (i / AffTile::H2) % AffTile::H1, h0 = i / (AffTile::H2 * AffTile::H1);
    const int p0 = b0 + h0 - 1, p1 = b1 + h1 - 1, p2 = b2 + h2 - 1;
    uint32_t v = 0x38u;                                       // out of the crop: identity of OR and AND
    if (p0 >= 0 && p0 < C0 && p1 >= 0 && p1 < C1 && p2 >= 0 && p2 < C2) {
      float q[3];
      v = 0u;
      if (res_coord<DISP>(S, T, disp, p0, p1, p2, h0, h1, h2, C0, C1, C2, c0, c1, c2, q)) {
        const int64_t s0 = S.o0 + (int64_t)floorf(__fadd_rn(q[0], 0.5f)), s1 = S.o1 + (int64_t)floorf(__fadd_rn(q[1], 0.5f)),
                      s2 = S.o2 + (int64_t)floorf(__fadd_rn(q[2], 0.5f));
        if (s0 >= 0 && s0 < S0 && s1 >= 0 && s1 < S1 && s2 >= 0 && s2 < S2) v = prep_bits(S.label[s0 * plane + s1 * S2 + s2]);
      }
    }
    H[h0][h1][h2] = (uint8_t)v;
  }

  // 2. image: eight dword taps per voxel and channel
  const bool inten = S.intensity != 0;
  const int64_t V_out = (int64_t)C0 * C1 * C2;
  float* xs = a.x + (int64_t)blockIdx.y * a.x_bs;
#pragma unroll 1
  for (int k = 0; k < AffTile::QUADS; ++k) {
    const int qd = tid + 256 * k;
    const int w = qd % AffTile::Q2, j = (qd / AffTile::Q2) % AffTile::T1, i = qd / (AffTile::Q2 * AffTile::T1);
    const int p0 = b0 + i, p1 = b1 + j, p2 = b2 + 4 * w;
    if (p0 >= C0 || p1 >= C1 || p2 >= C2) continue;
    const int64_t dst = ((int64_t)p0 * C1 + p1) * C2 + p2;
    float v[4][4];                                            // [channel][voxel of the quad]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float q[3];
      const bool ok = p2 + e < C2 && res_coord<DISP>(S, T, disp, p0, p1, p2 + e, i + 1, j + 1, 4 * w + e + 1, C0, C1, C2, c0, c1, c2, q);
      float fr[3] = {0.f, 0.f, 0.f};
      int64_t s[3] = {0, 0, 0};
      if (ok) {
        const int o[3] = {S.o0, S.o1, S.o2};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float fl = floorf(q[d]);
          fr[d] = __fsub_rn(q[d], fl);
          s[d] = o[d] + (int64_t)fl;
        }
      }
      const bool in0[2] = {ok && s[0] >= 0 && s[0] < S0, ok && s[0] + 1 >= 0 && s[0] + 1 < S0};
      const bool in1[2] = {s[1] >= 0 && s[1] < S1, s[1] + 1 >= 0 && s[1] + 1 < S1};
      const bool in2[2] = {s[2] >= 0 && s[2] < S2, s[2] + 1 >= 0 && s[2] + 1 < S2};
      const int64_t base = s[0] * plane + s[1] * S2 + s[2];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float* src = S.image + c * V + base;
        float r0[2];
#pragma unroll
        for (int d0 = 0; d0 < 2; ++d0) {
          float r1[2];
#pragma unroll
          for (int d1 = 0; d1 < 2; ++d1) {
            const bool row_in = in0[d0] && in1[d1];
            const float* row = src + d0 * plane + d1 * S2;
            const float t0 = (row_in && in2[0]) ? row[0] : 0.f;
            const float t1 = (row_in && in2[1]) ? row[1] : 0.f;
            r1[d1] = aff_lerp(t0, t1, fr[2]);
          }
          r0[d0] = aff_lerp(r1[0], r1[1], fr[1]);
        }
        float r = aff_lerp(r0[0], r0[1], fr[0]);
        if (inten) r = __fadd_rn(__fmul_rn(r, S.scale[c]), S.shift[c]);
        v[c][e] = r;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) prep_store_quad(xs + c * V_out + dst, v[c], a.vec, p2, C2);
  }
  __syncthreads();
  prep_tail<AffTile>(H, P1, P2, a, b0, b1, b2);
}

// ------------------------------------------------------------------------------------------------ the three entries
// what an entry asks of a sample beyond the common checks of prep_launch
static bool prep_all_finite(const float (&m)[9]) {
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(m[k])) return false;
  return true;
}
static bool prep_sample_ok(const cwf_prep_sample& s, const int (&C)[3]) {
  const int S[3] = {s.S0, s.S1, s.S2}, o[3] = {s.o0, s.o1, s.o2};
  for (int d = 0; d < 3; ++d)
    if (o[d] < 0 || o[d] > std::max(S[d] - C[d], 0)) return false;
  return true;
}
static bool prep_sample_ok(const cwf_prep_affine_sample& s, const int (&)[3]) { return prep_all_finite(s.m); }
static bool prep_sample_ok(const cwf_prep_elastic_sample& s, const int (&)[3]) {
  const int G[3] = {s.G0, s.G1, s.G2};
  for (int d = 0; d < 3; ++d)
    if (s.disp && (((uintptr_t)s.disp & 3) || G[d] < 4 || G[d] > ELA_GMAX)) return false;
  return prep_all_finite(s.m);
}

// the sample as the kernel takes it: the public struct itself, for the elastic kernel with what PrepElaSample adds
template <class Sample>
static void prep_pack(Sample& d, const Sample& s, const int (&)[3]) { d = s; }
static void prep_pack(PrepElaSample& d, const cwf_prep_elastic_sample& s, const int (&C)[3]) {
  static_cast<cwf_prep_elastic_sample&>(d) = s;
  if (!s.disp) d.G0 = d.G1 = d.G2 = 0;
  const int G[3] = {d.G0, d.G1, d.G2};
  for (int k = 0; k < 3; ++k) d.k[k] = (s.disp && C[k] > 1) ? (float)(G[k] - 3) / (float)(C[k] - 1) : 0.f;
}

// every entry: the argument checks (nothing is launched on a refusal), then one launch of kernel, which works on Tile, per eight samples
template <class Tile, class Sample, class HostSample>
static int prep_launch(void (*kernel)(PrepArgs<Sample>), const HostSample* h_samples, int B, int C0, int C1, int C2, float* x,
                       int64_t x_bstride, int64_t* target, int64_t t_bstride, int64_t* edge, int64_t e_bstride, void* stream) {
  if (!h_samples || B <= 0 || C0 <= 0 || C1 <= 0 || C2 <= 0 || !x || !target || !edge) return CWF_E_BADARG;
  const int64_t V = (int64_t)C0 * C1 * C2;
  if (V >= (int64_t(1) << 31)) return CWF_E_TOOLARGE;
  if (((uintptr_t)x & 3) || ((uintptr_t)target & 7) || ((uintptr_t)edge & 7)) return CWF_E_BADARG;
  if (x_bstride < 4 * V || t_bstride < V || e_bstride < V) return CWF_E_BADARG;
  const int C[3] = {C0, C1, C2};
  for (int b = 0; b < B; ++b) {
    const HostSample& s = h_samples[b];
    if (!s.image || !s.label || ((uintptr_t)s.image & 3) || s.flip < 0 || s.flip > 7) return CWF_E_BADARG;
    if (s.S0 <= 0 || s.S1 <= 0 || s.S2 <= 0 || !prep_sample_ok(s, C)) return CWF_E_BADARG;
  }
  PrepArgs<Sample> a;
  a.x_bs = x_bstride; a.t_bs = t_bstride; a.e_bs = e_bstride;
  a.C0 = C0; a.C1 = C1; a.C2 = C2;
  a.vec = (C2 % 4 == 0) && !((uintptr_t)x & 15) && !((uintptr_t)target & 15) && !((uintptr_t)edge & 15) && x_bstride % 4 == 0 &&
          t_bstride % 2 == 0 && e_bstride % 2 == 0;
  const int64_t tiles = (int64_t)cdiv(C0, Tile::T0) * cdiv(C1, Tile::T1) * cdiv(C2, Tile::T2);
  hipStream_t st = cwf_stream(stream);
  for (int b0 = 0; b0 < B; b0 += PREP_MAXS) {
    const int nb = std::min(PREP_MAXS, B - b0);
    for (int i = 0; i < PREP_MAXS; ++i) {
      if (i < nb) prep_pack(a.s[i], h_samples[b0 + i], C);
      else a.s[i] = Sample{};
    }
    a.x = x + (int64_t)b0 * x_bstride;
    a.target = target + (int64_t)b0 * t_bstride;
    a.edge = edge + (int64_t)b0 * e_bstride;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, (unsigned)nb), dim3(256), 0, st, a);
    CWF_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int cwf_prepare_batch(const struct cwf_prep_sample* h_samples, int B, int C0, int C1, int C2, float* x, int64_t x_bstride,
                                 int64_t* target, int64_t t_bstride, int64_t* edge, int64_t e_bstride, void* stream) {
  return prep_launch<PlainTile>(prep_batch_kernel, h_samples, B, C0, C1, C2, x, x_bstride, target, t_bstride, edge, e_bstride, stream);
}

extern "C" int cwf_prepare_batch_affine(const struct cwf_prep_affine_sample* h_samples, int B, int C0, int C1, int C2, float* x,
                                        int64_t x_bstride, int64_t* target, int64_t t_bstride, int64_t* edge, int64_t e_bstride,
                                        void* stream) {
  return prep_launch<AffTile>(prep_affine_kernel<cwf_prep_affine_sample>, h_samples, B, C0, C1, C2, x, x_bstride, target, t_bstride,
                              edge, e_bstride, stream);
}

extern "C" int cwf_prepare_batch_elastic(const struct cwf_prep_elastic_sample* h_samples, int B, int C0, int C1, int C2, float* x,
                                         int64_t x_bstride, int64_t* target, int64_t t_bstride, int64_t* edge, int64_t e_bstride,
                                         void* stream) {
  return prep_launch<AffTile>(prep_affine_kernel<PrepElaSample>, h_samples, B, C0, C1, C2, x, x_bstride, target, t_bstride, edge,
                              e_bstride, stream);
}

// ------------------------------------------------------------------------------------------------ brain-mask z-score
#define NORM_BLOCKS 512

__device__ __forceinline__ bool norm_mask(const float* __restrict__ x, int64_t v, int64_t V) {
  return __fadd_rn(__fadd_rn(__fadd_rn(x[v], x[V + v]), x[2 * V + v]), x[3 * V + v]) > 0.f;
}

// pass 0: partial (count, sum_c); pass 1: partial (count, sum_c (x - mean_c)^2).  ws[blk * 5 + {0: count, 1..4: channel}]
__global__ __launch_bounds__(256) void norm_partial_kernel(const float* __restrict__ x, int64_t V, double* __restrict__ ws, int pass) {
  __shared__ double red[4][5];
  const double* mean = ws + NORM_BLOCKS * 5;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    if (!norm_mask(x, v, V)) continue;
    acc[0] += 1.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double d = (double)x[c * V + v];
      if (pass == 0) {
        acc[1 + c] += d;
      } else {
        const double e = d - mean[c];
        acc[1 + c] += e * e;
      }
    }
  }
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double s = wave_sum_d(acc[k]);
    if (lane == 0) red[wv][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 5) ws[blockIdx.x * 5 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// one thread: reduce the partials in block order; pass 0 -> mean[4] (ws[NB*5 + 0..3]), pass 1 -> std[4] (ws[NB*5 + 4..7])
__global__ void norm_finalize_kernel(double* __restrict__ ws, int pass) {
  if (threadIdx.x != 0) return;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < NORM_BLOCKS; ++b)
    for (int k = 0; k < 5; ++k) s[k] += ws[b * 5 + k];
  double* out = ws + NORM_BLOCKS * 5 + (pass == 0 ? 0 : 4);
  for (int c = 0; c < 4; ++c) out[c] = s[0] > 0.0 ? (pass == 0 ? s[1 + c] / s[0] : sqrt(s[1 + c] / s[0])) : 0.0;
}

__global__ __launch_bounds__(256) void norm_apply_kernel(float* __restrict__ x, int64_t V, const double* __restrict__ ws) {
  const double* mean = ws + NORM_BLOCKS * 5;
  const double* sd = mean + 4;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    if (!norm_mask(x, v, V)) continue;
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = sd[c] > 0.0 ? (float)(((double)x[c * V + v] - mean[c]) / sd[c]) : x[c * V + v];
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c * V + v] = r[c];
  }
}

extern "C" int cwf_normalize_nonzero(float* image, int64_t V, double* ws, void* stream) {
  if (!image || !ws || V <= 0 || ((uintptr_t)image & 3) || ((uintptr_t)ws & 7)) return CWF_E_BADARG;
  hipStream_t st = cwf_stream(stream);
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(norm_partial_kernel, dim3(NORM_BLOCKS), dim3(256), 0, st, (const float*)image, V, ws, pass);
    CWF_LAUNCH_CHECK();
    hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(64), 0, st, ws, pass);
    CWF_LAUNCH_CHECK();
  }
  const int nb = (int)std::min<int64_t>(cdiv64(V, 256), 4096);
  hipLaunchKernelGGL(norm_apply_kernel, dim3(nb), dim3(256), 0, st, image, V, (const double*)ws);
  CWF_LAUNCH_CHECK();
  return 0;
}
