// prefix.h — the CACHED prefix of the 3-D AMOS trainer on the device (train_inherent_consistent_unet_3D_AMOS22.py:86-101 and, for
// validation, :141-154):  ScaleIntensityRanged -> CropForegroundd -> Orientationd("RAS") -> [SpatialPadd] -> Spacingd, and its inverse
// for label maps.  The definition (DESIGN.md "AMOS cached prefix"; restated literally in tests/amos_prefix_ref.py):
//   window, per raw voxel, fp32, every operation rounded on its own:  t = (v - a_min) / a_range;  t = t * b_range + b_min;
//       with clip: t = min(max(t, b_min), b_max)   (a NaN stays a NaN)
//   box:      the smallest box of the raw volume that holds every voxel with t > 0
//   orient:   oriented axis a is raw axis perm[a] of the box, reversed when sign[a] < 0
//   pad:      f_a zeros in front of oriented axis a, the padded extent is m_a (image 0.0, label 0)
//   respace:  per axis x = min(max(j * (p / s), 0), m - 1) in double;  image: i0 = floor(x), f = x - i0, i1 = min(i0 + 1, m - 1), the eight
//       taps (0,0,0), (0,0,1), ..., (1,1,1) as double(tap) * ((w_0 * w_1) * w_2), summed left to right in double, rounded once to fp32;
//       label: the voxel at rint(x) per axis (half to even)
// Window and orient..respace compose into ONE gather from the raw arrays: no intermediate volume exists.  Every coordinate is fp64
// with contraction off (`fp contract(off)`, as the 2-D slice gather of datafeed.h), so that the GPU, the emulation and numpy perform the
// same IEEE operations.  No atomics anywhere: the box is reduced per workgroup into a workspace and finished by one workgroup in a
// fixed order.
#pragma once

namespace icl {

constexpr int kPrefixThreads = 256;
constexpr int kPrefixBoxBlocks = 1024;      // most partial boxes of one volume: the workspace holds 6 int32 each
constexpr int kPrefixIntMax = 0x7fffffff;

struct PrefixWindow {
  float a_min, a_range;      // a_range = fp32(a_max - a_min), the difference formed in double by the host
  float b_min, b_range;      // b_range = fp32(b_max - b_min)
  float b_max;
  int clip;
};

// ScaleIntensityRange of one voxel: three (five with clip) fp32 operations, each rounded on its own
__device__ __forceinline__ float prefix_window(float v, const PrefixWindow& w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float t = v - w.a_min;
  t = t / w.a_range;
  t = t * w.b_range;
  t = t + w.b_min;
  if (w.clip) {
    t = t < w.b_min ? w.b_min : t;
    t = t > w.b_max ? w.b_max : t;
  }
  return t;
}

// The workgroup's box from every thread's: lo[a] = min, hi[a] = max (inclusive) per axis; thread 0 stores the six integers to `out`.
// Integer min / max only, the four waves combined in index order.  `part`: 6 * kPrefixThreads / 64 words of LDS.  One barrier inside.
__device__ __forceinline__ void prefix_box_reduce(int lo[3], int hi[3], int* part, int* __restrict__ out) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int l = __shfl_down(lo[a], d, 64), h = __shfl_down(hi[a], d, 64);
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      part[wave * 6 + a] = lo[a];
      part[wave * 6 + 3 + a] = hi[a];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int l = part[a], h = part[3 + a];
#pragma unroll
      for (int w = 1; w < kPrefixThreads / 64; ++w) {
        l = part[w * 6 + a] < l ? part[w * 6 + a] : l;
        h = part[w * 6 + 3 + a] > h ? part[w * 6 + 3 + a] : h;
      }
      out[a] = l;
      out[3 + a] = h;
    }
  }
}

// grid (G <= kPrefixBoxBlocks), kPrefixThreads threads.  image [n0][n1][n2] fp32; ws [G][6] int32: workgroup g's {lo0, lo1, lo2, hi0, hi1,
// hi2} over the voxels it visited whose windowed value is > 0 (lo = INT_MAX, hi = -1 where it saw none).  One thread per four
// consecutive flat voxels; vec: the image is 16-byte aligned, so a whole group is one 16-byte load.
__global__ __launch_bounds__(kPrefixThreads) void prefix_box_partial_kernel(const float* __restrict__ image, int n1, int n2, long total,
                                                                            PrefixWindow win, int vec, int* __restrict__ ws) {
  __shared__ int part[6 * kPrefixThreads / 64];
  int lo[3] = {kPrefixIntMax, kPrefixIntMax, kPrefixIntMax}, hi[3] = {-1, -1, -1};
  const unsigned groups = (unsigned)((total + 3) / 4);                        // the launcher keeps total below 2^31
  for (unsigned q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
    const long first = (long)q * 4;
    float x[4];
    bool in[4];
    if (vec && first + 4 <= total) {
      const float4 v = *reinterpret_cast<const float4*>(image + first);
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
      in[0] = in[1] = in[2] = in[3] = true;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        in[t] = first + t < total;
        x[t] = in[t] ? image[first + t] : 0.f;
      }
    }
    int i2 = (int)((unsigned)first % (unsigned)n2);
    const unsigned row = (unsigned)first / (unsigned)n2;
    int i1 = (int)(row % (unsigned)n1), i0 = (int)(row / (unsigned)n1);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (in[t] && prefix_window(x[t], win) > 0.f) {      // NaN > 0 is false
        lo[0] = i0 < lo[0] ? i0 : lo[0]; hi[0] = i0 > hi[0] ? i0 : hi[0];
        lo[1] = i1 < lo[1] ? i1 : lo[1]; hi[1] = i1 > hi[1] ? i1 : hi[1];
        lo[2] = i2 < lo[2] ? i2 : lo[2]; hi[2] = i2 > hi[2] ? i2 : hi[2];
      }
      if (++i2 == n2) {
        i2 = 0;
        if (++i1 == n1) { i1 = 0; ++i0; }
      }
    }
  }
  prefix_box_reduce(lo, hi, part, ws + 6 * blockIdx.x);
}

// grid (1), kPrefixThreads threads: the box of `count` partial boxes, box [6] int32 = {lo0, lo1, lo2, hi0, hi1, hi2}, hi INCLUSIVE; an
// empty foreground leaves lo = INT_MAX and hi = -1.
__global__ __launch_bounds__(kPrefixThreads) void prefix_box_finish_kernel(const int* __restrict__ ws, int count, int* __restrict__ box) {
  __shared__ int part[6 * kPrefixThreads / 64];
  int lo[3] = {kPrefixIntMax, kPrefixIntMax, kPrefixIntMax}, hi[3] = {-1, -1, -1};
  for (int g = threadIdx.x; g < count; g += kPrefixThreads) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int l = ws[6 * g + a], h = ws[6 * g + 3 + a];
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
  }
  prefix_box_reduce(lo, hi, part, box);
}

// The composed map of one case, made by the launcher from a checked plan.  Oriented axis a: crop index c (0 <= c < e[a]) is the raw
// voxel at offset base + c * step[a] along that axis (step carries the raw stride of axis perm[a] and the sign of the reversal).
struct PrefixGeom {
  long base;               // flat raw offset of the oriented crop's voxel (0, 0, 0)
  long step[3];            // flat raw stride of one step along oriented axis a (negative when reversed)
  int e[3];                // extents of the oriented crop
  int f[3];                // zeros in front of it (SpatialPad)
  int m[3];                // padded extents, m >= f + e
  int o[3];                // output extents
  double fwd[3];           // p / s: oriented coordinate of output index j is j * fwd
};

// The inverse map, per RAW axis k (a = the oriented axis with perm[a] == k), made by the launcher from the same checked plan.
struct PrefixRestoreGeom {
  int n[3];                // raw extents
  int lo[3], hi[3];        // the box, hi exclusive
  int rev[3];              // oriented axis a is reversed
  int f[3];                // zeros in front of oriented axis a
  int o[3];                // extent of the prediction along oriented axis a
  long pstride[3];         // flat stride of the prediction along oriented axis a
  double inv[3];           // s / p of oriented axis a: output coordinate of padded oriented index u is u * inv
};

struct PrefixTap {
  long off0, off1;         // raw offsets (relative to base) of the two taps along one axis ...
  int in0, in1;            // ... which lie in the crop (0: in the pad, the offset is 0 and not used)
  double w0, w1;
  long offn;               // the nearest voxel (label)
  int inn;
  int i0, i1;              // the two taps' indices in the padded oriented grid
};

// taps of output index j along oriented axis a
__device__ __forceinline__ PrefixTap prefix_tap(const PrefixGeom& g, int a, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double top = (double)(g.m[a] - 1);
  double x = (double)j * g.fwd[a];
  x = x < 0.0 ? 0.0 : x;
  x = x > top ? top : x;
  const double fl = floor(x);
  const double f = x - fl;
  const int i0 = (int)fl;
  const int i1 = i0 + 1 < g.m[a] ? i0 + 1 : g.m[a] - 1;
  const int in_ = (int)rint(x);                      // half to even
  PrefixTap t;
  t.i0 = i0;
  t.i1 = i1;
  t.w0 = 1.0 - f;
  t.w1 = f;
  const int c0 = i0 - g.f[a], c1 = i1 - g.f[a], cn = in_ - g.f[a];
  t.in0 = c0 >= 0 && c0 < g.e[a];
  t.in1 = c1 >= 0 && c1 < g.e[a];
  t.inn = cn >= 0 && cn < g.e[a];
  t.off0 = t.in0 ? (long)c0 * g.step[a] : 0;
  t.off1 = t.in1 ? (long)c1 * g.step[a] : 0;
  t.offn = t.inn ? (long)cn * g.step[a] : 0;
  return t;
}

// image_out [o0][o1][o2] fp32, label_out [o0][o1][o2] uint8, both written by one launch: a thread's coordinates serve both.  One
// thread per V consecutive outputs along oriented axis 2 (V = 4: o2 % 4 == 0, image_out 16-byte and label_out 4-byte aligned: one
// 16-byte and one 4-byte store).
//
// A workgroup owns a tile of one j0, kPrefixRows consecutive j1 and `tile2` consecutive j2.  Along oriented axis 2 neighbouring outputs
// share their taps (AMOS upsamples that axis 2.5 times), and the window costs an IEEE division: so the tile's source rows — 4 per j1,
// the (i0 | i1) x (i0 | i1) taps of axes 0 and 1 — are windowed ONCE into LDS over the span of axis-2 taps the tile needs (a pad tap is
// stored as 0.0, NOT the window of 0), a wave per row and a lane per slot, and the outputs then take their eight taps from LDS.  Same
// operations on the same values as tap by tap, so the result is the same bit for bit.  The launcher chooses tile2 such that the span
// fits kPrefixSlots; the kernel clamps it all the same, so that no tile2 can send an access outside the LDS rows.  With oriented axis
// 2 = raw axis 2 (what AMOS files give) a wave reads along the raw volume's fastest axis; the other permutations run the same code
// with strided reads.  Every tap is read inside the box: a pad tap is never dereferenced.
constexpr int kPrefixRows = 8;        // j1 rows per tile
constexpr int kPrefixSlots = 256;     // most axis-2 taps a tile may span
constexpr int kPrefixTile2 = 512;     // most axis-2 outputs per tile

template <int V>
__global__ __launch_bounds__(kPrefixThreads) void prefix_resample_kernel(const float* __restrict__ image, const uint8_t* __restrict__ label,
                                                                         PrefixGeom g, PrefixWindow win, int tile2,
                                                                         float* __restrict__ image_out, uint8_t* __restrict__ label_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  static_assert(V == 1 || V == 4, "one voxel or one quad per thread");
  __shared__ float rows[kPrefixRows * 4 * kPrefixSlots];
  const float* __restrict__ src = image + g.base;
  const uint8_t* __restrict__ lab = label + g.base;
  const unsigned nt2 = (unsigned)((g.o[2] + tile2 - 1) / tile2), nt1 = (unsigned)((g.o[1] + kPrefixRows - 1) / kPrefixRows);
  const unsigned ntiles = (unsigned)g.o[0] * nt1 * nt2;                       // at most o0 * o1 * o2, which the launcher keeps below 2^31
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {        // the same trip count for every thread: barriers inside
    const int j2base = (int)(tile % nt2) * tile2;
    const unsigned trest = tile / nt2;
    const int j1base = (int)(trest % nt1) * kPrefixRows, j0 = (int)(trest / nt1);
    const int j2end = j2base + tile2 < g.o[2] ? j2base + tile2 : g.o[2];
    const PrefixTap t0 = prefix_tap(g, 0, j0);
    const int slot0 = prefix_tap(g, 2, j2base).i0;                            // the coordinate does not fall as j grows
    int span = prefix_tap(g, 2, j2end - 1).i1 - slot0 + 1;
    span = span > kPrefixSlots ? kPrefixSlots : span;
    for (int row = wave; row < kPrefixRows * 4; row += kPrefixThreads / 64) { // row = 4 * (j1 - j1base) + 2 * (tap of axis 0) + (tap of axis 1)
      const int j1 = j1base + (row >> 2);
      if (j1 >= g.o[1]) break;
      const PrefixTap t1 = prefix_tap(g, 1, j1);
      const bool in01 = ((row & 2) ? t0.in1 : t0.in0) && ((row & 1) ? t1.in1 : t1.in0);
      const long off01 = ((row & 2) ? t0.off1 : t0.off0) + ((row & 1) ? t1.off1 : t1.off0);
      for (int s = lane; s < span; s += 64) {
        const int c2 = slot0 + s - g.f[2];
        float x = 0.f;
        if (in01 && c2 >= 0 && c2 < g.e[2]) x = prefix_window(src[off01 + (long)c2 * g.step[2]], win);
        rows[row * kPrefixSlots + s] = x;
      }
    }
    __syncthreads();
    const int q2 = (j2end - j2base + V - 1) / V;                              // V = 4: o2 and tile2 are multiples of 4, so is every tile
    for (int item = threadIdx.x; item < kPrefixRows * q2; item += kPrefixThreads) {
      const int r1 = item / q2, j2 = j2base + (item % q2) * V, j1 = j1base + r1;
      if (j1 >= g.o[1]) break;
      const PrefixTap t1 = prefix_tap(g, 1, j1);
      const double w00 = t0.w0 * t1.w0, w01 = t0.w0 * t1.w1, w10 = t0.w1 * t1.w0, w11 = t0.w1 * t1.w1;
      const float* __restrict__ r00 = rows + (r1 * 4 + 0) * kPrefixSlots;
      const float* __restrict__ r01 = rows + (r1 * 4 + 1) * kPrefixSlots;
      const float* __restrict__ r10 = rows + (r1 * 4 + 2) * kPrefixSlots;
      const float* __restrict__ r11 = rows + (r1 * 4 + 3) * kPrefixSlots;
      float v[V];
      unsigned lv[V];
#pragma unroll
      for (int t = 0; t < V; ++t) {
        const PrefixTap t2 = prefix_tap(g, 2, j2 + t);
        int s0 = t2.i0 - slot0, s1 = t2.i1 - slot0;
        s0 = s0 < kPrefixSlots ? s0 : kPrefixSlots - 1;
        s1 = s1 < kPrefixSlots ? s1 : kPrefixSlots - 1;
        // the eight taps in the order (0,0,0), (0,0,1), (0,1,0), ..., (1,1,1)
        const double x000 = (double)r00[s0], x001 = (double)r00[s1], x010 = (double)r01[s0], x011 = (double)r01[s1];
        const double x100 = (double)r10[s0], x101 = (double)r10[s1], x110 = (double)r11[s0], x111 = (double)r11[s1];
        double acc = x000 * (w00 * t2.w0);
        acc = acc + x001 * (w00 * t2.w1);
        acc = acc + x010 * (w01 * t2.w0);
        acc = acc + x011 * (w01 * t2.w1);
        acc = acc + x100 * (w10 * t2.w0);
        acc = acc + x101 * (w10 * t2.w1);
        acc = acc + x110 * (w11 * t2.w0);
        acc = acc + x111 * (w11 * t2.w1);
        v[t] = (float)acc;
        lv[t] = t0.inn && t1.inn && t2.inn ? (unsigned)lab[t0.offn + t1.offn + t2.offn] : 0u;
      }
      const long e = ((long)j0 * g.o[1] + j1) * g.o[2] + j2;
      if constexpr (V == 4) {
        *reinterpret_cast<float4*>(image_out + e) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<unsigned*>(label_out + e) = lv[0] | (lv[1] << 8) | (lv[2] << 16) | (lv[3] << 24);
      } else {
        image_out[e] = v[0];
        label_out[e] = (uint8_t)lv[0];
      }
    }
    __syncthreads();                                                          // the rows are written again for the next tile
  }
}

// The inverse for label maps (what MONAI's Invertd does to a prediction): out [n0][n1][n2] uint8 on the RAW grid.  Outside the box 0;
// inside, raw voxel -> oriented crop index -> padded index u -> y = min(max(u * (s / p), 0), o - 1) -> pred[rint(y)].  T: the
// prediction's element (uint8_t or long long; the low byte is kept).  One thread per raw voxel, raw axis 2 fastest.
template <typename T>
__global__ __launch_bounds__(kPrefixThreads) void prefix_restore_kernel(const T* __restrict__ pred, PrefixRestoreGeom g,
                                                                        uint8_t* __restrict__ out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const unsigned total = (unsigned)g.n[0] * g.n[1] * g.n[2];                  // the launcher keeps it below 2^31
  for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < total; r += gridDim.x * blockDim.x) {
    int idx[3];
    idx[2] = (int)(r % (unsigned)g.n[2]);
    const unsigned rest = r / (unsigned)g.n[2];
    idx[1] = (int)(rest % (unsigned)g.n[1]);
    idx[0] = (int)(rest / (unsigned)g.n[1]);
    bool inside = true;
    long at = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      inside = inside && idx[k] >= g.lo[k] && idx[k] < g.hi[k];
      int c = idx[k] - g.lo[k];
      if (g.rev[k]) c = g.hi[k] - g.lo[k] - 1 - c;
      const double top = (double)(g.o[k] - 1);
      double y = (double)(c + g.f[k]) * g.inv[k];
      y = y < 0.0 ? 0.0 : y;                                                    // also every voxel outside the box, which is not read
      y = y > top ? top : y;
      at += (long)rint(y) * g.pstride[k];                                       // half to even
    }
    uint8_t v = 0;
    if (inside) v = (uint8_t)pred[at];
    out[r] = v;
  }
}

}  // namespace icl
