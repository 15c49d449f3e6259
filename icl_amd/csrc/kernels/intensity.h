// intensity.h — the INTENSITY stage of the 3-D device feed: Gaussian noise, Gaussian blur, simulated low resolution, contrast and gamma on the image batch
// [B][1][R0][R1][R2] fp32 that the geometric gather (datafeed.h) has written.  nnU-Net's GaussianNoise / GaussianBlur / ContrastAugmentation /
// Gamma transforms, MONAI's RandGaussianNoised / RandGaussianSmoothd / RandAdjustContrastd and the reference's RandomNoise
// (dataloaders/brats2019.py:150-161).  The definition is in DESIGN.md §2 "Intensity stage of the 3-D feed"; tests/intensity_feed_ref.py
// restates it in numpy.  Per sample, in this order, each transform only where the sample drew it (one sample per blockIdx.y: the flag is
// wave-uniform and a sample without the transform leaves at once):
//   noise     x = fp32(x + n),  n = fp32(sigma z) clipped to +-limit,  z = sqrt(-2 ln u1) cos(2 pi u2) in double,
//             h1 = mix32(i * 0x9E3779B1 + seed), h2 = mix32(h1 + 0x632BE5AB), u1 = (h1 + 0.5) / 2^32, u2 = h2 / 2^32, i the flat voxel index
//             within the sample: one pair of uniforms serves ONE voxel (the sine partner is not used), so a voxel's variate depends on
//             (seed, i) alone and not on how the voxels are spread over threads
//   blur      scipy.ndimage.gaussian_filter(x, sigma, mode="reflect", truncate=4.0): axes 0, 1, 2 in turn, each pass reading the previous
//             pass's fp32 result; per output, in double, acc = w_0 x[c], then acc = acc + (x[c - k] + x[c + k]) w_k for k = 1 .. r, rounded
//             once to fp32; an index outside the patch is reflected about the edge (d c b a | a b c d | d c b a); the weights come from the host
//   lowres    (off unless asked for) nnU-Net's SimulateLowResolutionTransform as two interpolate calls, "nearest-exact" down to the low
//             extents L and "trilinear" back up, as one gather of 8 patch voxels per output: the formulas are at lowres_near / lowres_tap
//             and the value at intensity_lowres_kernel; batch -> scratch, and a second launch copies the samples that drew it back
//   stats     min, max (exact) and mean = fp32(double sum / N) of the sample, the sum in the fixed order given at the kernels
//   contrast  y = fp32(fp32(fp32(x - mean) f) + mean), clipped to [min, max]
//   gamma     on the result of contrast, whose extremes mn, mx are the images of min and max (the map is monotone); with invert x -> -x
//             before and after; in double t = (x - mn) / ((mx - mn) + 1e-7), p = t when g = 1 and pow(t, g) otherwise,
//             y = fp32(fp32(p (mx - mn)) + mn), the product and the sum formed in double
// fp contraction is off in every function that rounds; no atomics; no float reduction whose order depends on scheduling.
#pragma once

namespace icl {

constexpr int kIntensityThreads = 256;
constexpr int kBlurMaxRadius = 12;           // r = int(4 sigma + 0.5) <= 12 covers sigma <= 3
constexpr int kBlurTileL = 32;               // strided passes: outputs along the filtered axis per tile
constexpr int kBlurTileI = 32;               // strided passes: contiguous columns per tile (128 B a row)
constexpr int kBlurLineFloats = 4096;        // contiguous pass: floats of whole lines staged per workgroup (and the largest R2 it takes)
constexpr int kIntensityStatBlocks = 64;     // most partial sums per sample

struct NoiseSample {
  int on;                    // 1: the sample drew noise
  unsigned seed;
  double sigma;
  int clip;                  // 1: n is clipped to [-limit, limit]
  float limit;               // fp32(clip * sigma), formed in double by the launcher
};
struct NoiseBatch {
  NoiseSample s[kFeedMaxBatch];      // 24 B a record
};

// the variate of voxel i of a sample: see the head of this file
__device__ __forceinline__ float intensity_noise_value(const NoiseSample& s, unsigned i) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const unsigned h1 = mix32(i * 0x9E3779B1u + s.seed);
  const unsigned h2 = mix32(h1 + 0x632BE5ABu);
  const double u1 = ((double)h1 + 0.5) * (1.0 / 4294967296.0);      // exact
  const double u2 = (double)h2 * (1.0 / 4294967296.0);              // exact
  const double rad = sqrt(-2.0 * log(u1));
  const double z = rad * cos(6.283185307179586 * u2);
  float n = (float)(s.sigma * z);
  if (s.clip) {
    n = n < -s.limit ? -s.limit : n;
    n = n > s.limit ? s.limit : n;
  }
  return n;
}

// grid (x, B), 256 threads.  image [B][per] fp32, in place.  V = 4: per % 4 == 0 and the batch is 16-byte aligned, one 16-byte load and
// store per thread and step; V = 1: one voxel.  No LDS.
template <int V>
__global__ __launch_bounds__(kIntensityThreads) void intensity_noise_kernel(NoiseBatch nb, float* __restrict__ image, unsigned per) {
  static_assert(V == 1 || V == 4, "one voxel or one quad per thread");
  const int b = blockIdx.y;
  const NoiseSample& s = nb.s[b];
  if (!s.on) return;
  float* __restrict__ x = image + (long)b * per;
  const unsigned groups = per / V;
  for (unsigned q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
    if constexpr (V == 4) {
      float4 v = *reinterpret_cast<const float4*>(x + (long)q * 4);
      v.x = v.x + intensity_noise_value(s, q * 4);
      v.y = v.y + intensity_noise_value(s, q * 4 + 1);
      v.z = v.z + intensity_noise_value(s, q * 4 + 2);
      v.w = v.w + intensity_noise_value(s, q * 4 + 3);
      *reinterpret_cast<float4*>(x + (long)q * 4) = v;
    } else {
      x[q] = x[q] + intensity_noise_value(s, q);
    }
  }
}

struct BlurSample {
  int on;                               // 1: the sample drew a blur with r >= 1 (r = 0 is the identity and is not launched)
  int r;                                // 1 .. kBlurMaxRadius, and at most the smallest patch extent
  double w[kBlurMaxRadius + 1];         // w_0 .. w_r, normalised, from the host
};
struct BlurBatch {
  BlurSample s[kFeedMaxBatch];          // 112 B a record: 1,792 B of the 4 KB kernel-argument block
};

// scipy's "reflect": (d c b a | a b c d | d c b a).  The launcher keeps r <= n, so one reflection brings every index into [0, n - 1].
__device__ __forceinline__ int blur_reflect(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

// One pass along a STRIDED axis (axis 0: outer = 1, n = R0, inner = R1 R2; axis 1: outer = R0, n = R1, inner = R2), src -> dst, both
// [B][outer][n][inner] fp32 and distinct.  grid (x, B), 256 threads = 32 columns x 8 row groups.  A tile is kBlurTileL outputs along the axis
// by kBlurTileI contiguous columns; its rows and the r reflected or neighbouring rows on either side go through LDS once (7 KB), so a value
// is read from memory once per tile and not 2 r + 1 times; lanes of a wave read consecutive columns of two LDS rows: no bank conflict.
__global__ __launch_bounds__(kIntensityThreads) void intensity_blur_strided_kernel(BlurBatch bb, const float* __restrict__ src,
                                                                                   float* __restrict__ dst, int outer, int n, int inner,
                                                                                   unsigned per) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  __shared__ float tile[(kBlurTileL + 2 * kBlurMaxRadius) * kBlurTileI];
  __shared__ double wsh[kBlurMaxRadius + 1];
  const int b = blockIdx.y;
  const BlurSample& s = bb.s[b];
  if (!s.on) return;
  const int r = s.r;
  if ((int)threadIdx.x <= r) wsh[threadIdx.x] = s.w[threadIdx.x];
  const int tl = (n + kBlurTileL - 1) / kBlurTileL, ti = (inner + kBlurTileI - 1) / kBlurTileI;
  const unsigned tiles = (unsigned)outer * tl * ti;                             // at most per: below 2^31
  const float* __restrict__ xs = src + (long)b * per;
  float* __restrict__ xd = dst + (long)b * per;
  const int col = threadIdx.x & (kBlurTileI - 1), rg = threadIdx.x / kBlurTileI;
  constexpr int kGroups = kIntensityThreads / kBlurTileI;
  for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int it = (int)(t % ti);
    const unsigned rest = t / ti;
    const int lt = (int)(rest % tl), o = (int)(rest / tl);
    const int l0 = lt * kBlurTileL, c = it * kBlurTileI + col;
    const int nl = n - l0 < kBlurTileL ? n - l0 : kBlurTileL;
    const long base = (long)o * n * inner;
    if (c < inner)
      for (int j = rg; j < nl + 2 * r; j += kGroups) tile[j * kBlurTileI + col] = xs[base + (long)blur_reflect(l0 - r + j, n) * inner + c];
    __syncthreads();
    if (c < inner) {
      for (int j = rg; j < nl; j += kGroups) {
        const float* p = tile + (j + r) * kBlurTileI + col;
        double acc = wsh[0] * (double)p[0];
        for (int k = 1; k <= r; ++k) acc = acc + ((double)p[-k * kBlurTileI] + (double)p[k * kBlurTileI]) * wsh[k];
        xd[base + (long)(l0 + j) * inner + c] = (float)acc;
      }
    }
    __syncthreads();
  }
}

// The pass along the CONTIGUOUS axis, in place: image [B][lines][n] fp32, n = R2 <= kBlurLineFloats, lines = R0 R1.  grid (x, B), 256
// threads.  A workgroup owns `lpb` consecutive whole lines at a time (lpb n <= kBlurLineFloats floats, one contiguous piece of memory):
// it copies them into LDS, and only after the barrier behind the last read does it compute (thread e, e + 256, ...: consecutive LDS words,
// no bank conflict at the centre tap) into a second LDS buffer, which it then copies back over the lines it read.  No other workgroup
// touches those lines, so nothing is read after it was overwritten.  V = 4: n % 4 == 0 and the batch is 16-byte aligned, the two copies
// move 16 bytes a thread; V = 1: 4 bytes.  32 KB of LDS.
template <int V>
__global__ __launch_bounds__(kIntensityThreads) void intensity_blur_line_kernel(BlurBatch bb, float* __restrict__ image, int lines, int n,
                                                                                int lpb, unsigned per) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  static_assert(V == 1 || V == 4, "4 or 16 bytes per thread");
  __shared__ float in[kBlurLineFloats] __attribute__((aligned(16)));
  __shared__ float out[kBlurLineFloats] __attribute__((aligned(16)));
  __shared__ double wsh[kBlurMaxRadius + 1];
  const int b = blockIdx.y;
  const BlurSample& s = bb.s[b];
  if (!s.on) return;
  const int r = s.r;
  if ((int)threadIdx.x <= r) wsh[threadIdx.x] = s.w[threadIdx.x];
  float* __restrict__ x = image + (long)b * per;
  const int chunks = (lines + lpb - 1) / lpb;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int l0 = ch * lpb;
    const int nl = lines - l0 < lpb ? lines - l0 : lpb;
    const int count = nl * n;                                                   // <= kBlurLineFloats
    float* __restrict__ g = x + (long)l0 * n;
    if constexpr (V == 4) {
      for (int q = threadIdx.x; q < count / 4; q += kIntensityThreads)
        reinterpret_cast<float4*>(in)[q] = reinterpret_cast<const float4*>(g)[q];
    } else {
      for (int e = threadIdx.x; e < count; e += kIntensityThreads) in[e] = g[e];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < count; e += kIntensityThreads) {
      const int line = e / n, c = e - line * n;
      const float* p = in + line * n;
      double acc = wsh[0] * (double)p[c];
      for (int k = 1; k <= r; ++k) acc = acc + ((double)p[blur_reflect(c - k, n)] + (double)p[blur_reflect(c + k, n)]) * wsh[k];
      out[e] = (float)acc;
    }
    __syncthreads();
    if constexpr (V == 4) {
      for (int q = threadIdx.x; q < count / 4; q += kIntensityThreads)
        reinterpret_cast<float4*>(g)[q] = reinterpret_cast<const float4*>(out)[q];
    } else {
      for (int e = threadIdx.x; e < count; e += kIntensityThreads) g[e] = out[e];
    }
    // the next round writes `in` (last read before the barrier above) and writes `out` only behind its own first barrier
  }
}

struct LowresSample {
  int on;                    // 1: the sample drew low resolution and some L[a] < R[a] (all equal is the identity and is not launched)
  int L[3];                  // low extents, 1 <= L[a] <= R[a]
  float sn[3];               // fp32(R[a]) / fp32(L[a]), formed by the launcher
  float sl[3];               // fp32(L[a]) / fp32(R[a]), formed by the launcher
};
struct LowresBatch {
  LowresSample s[kFeedMaxBatch];        // 40 B a record
};

// the patch voxel that low-resolution cell i stands for (interpolate's "nearest-exact"): min(floor(fp32(fp32(i + 0.5) sn)), R - 1)
__device__ __forceinline__ int lowres_near(int i, float sn, int R) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float c = (float)i + 0.5f;                                              // exact below 2^23
  const float p = c * sn;                                                       // >= 0: the conversion below is the floor
  const int v = p < 2147483648.f ? (int)p : R - 1;                              // 2^31 and above is beyond every R - 1
  return v < R - 1 ? v : R - 1;
}

struct LowresTap {
  int s0, s1;                // the two patch voxels along one axis
  float w0, w1;              // their weights
};

// one axis of output index o (interpolate's "linear" with align_corners=False on the low-resolution cells, then lowres_near): src is
// sl (o + 0.5) - 0.5 rounded ONCE (one fma), negative -> 0; i0 = min(int(src), L - 1), i1 = i0 + (i0 < L - 1); w1 = src - i0 clipped to
// [0, 1], w0 = 1 - w1.  Both voxels lie in [0, R - 1] whatever the arguments.
__device__ __forceinline__ LowresTap lowres_tap(int o, int L, int R, float sn, float sl) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float src = fmaf(sl, (float)o + 0.5f, -0.5f);
  src = src < 0.f ? 0.f : src;
  int i0 = src < 2147483648.f ? (int)src : L - 1;
  i0 = i0 < L - 1 ? i0 : L - 1;
  const int i1 = i0 + (i0 < L - 1 ? 1 : 0);
  float w1 = src - (float)i0;
  w1 = w1 < 0.f ? 0.f : w1;
  w1 = w1 > 1.f ? 1.f : w1;
  LowresTap t;
  t.s0 = lowres_near(i0, sn, R);
  t.s1 = lowres_near(i1, sn, R);
  t.w0 = 1.f - w1;
  t.w1 = w1;
  return t;
}

// a v0 + b v1 in double, the two products rounded (exact when a and b came from fp32 values), then the sum
__device__ __forceinline__ double lowres_mix(double a, float v0, double b, float v1) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double p = a * (double)v0;
  const double q = b * (double)v1;
  return p + q;
}

// Simulated low resolution (nnU-Net's SimulateLowResolutionTransform as batchgeneratorsv2 defines it: interpolate "nearest-exact" down
// to L, "trilinear" back up to R) as ONE gather: src -> dst, both [B][R0][R1][R2] fp32 and distinct; the low-resolution volume is never
// written, each output reads the 8 patch voxels its 8 low-resolution cells stand for.  grid (x, B), 256 threads.  V = 4: R2 % 4 == 0 and
// dst is 16-byte aligned, a thread forms the four outputs of one quad along axis 2 (they share the taps of axes 0 and 1) and writes 16
// bytes; V = 1: one voxel.  The value: along axis 2, then 1, then 0, in double, one rounding to fp32 at the end.  No LDS.
template <int V>
__global__ __launch_bounds__(kIntensityThreads) void intensity_lowres_kernel(LowresBatch lb, const float* __restrict__ src,
                                                                             float* __restrict__ dst, int R0, int R1, int R2, unsigned per) {
  static_assert(V == 1 || V == 4, "one voxel or one quad per thread");
  const int b = blockIdx.y;
  const LowresSample& s = lb.s[b];
  if (!s.on) return;
  const float* __restrict__ x = src + (long)b * per;
  float* __restrict__ y = dst + (long)b * per;
  const unsigned row = (unsigned)R2 / V;                                        // groups along axis 2
  const unsigned groups = per / V;
  for (unsigned q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
    const unsigned line = q / row;
    const int o2 = (int)(q - line * row) * V;
    const int o0 = (int)(line / (unsigned)R1), o1 = (int)(line - (unsigned)o0 * (unsigned)R1);
    const LowresTap t0 = lowres_tap(o0, s.L[0], R0, s.sn[0], s.sl[0]);
    const LowresTap t1 = lowres_tap(o1, s.L[1], R1, s.sn[1], s.sl[1]);
    const float* __restrict__ p00 = x + ((long)t0.s0 * R1 + t1.s0) * R2;
    const float* __restrict__ p01 = x + ((long)t0.s0 * R1 + t1.s1) * R2;
    const float* __restrict__ p10 = x + ((long)t0.s1 * R1 + t1.s0) * R2;
    const float* __restrict__ p11 = x + ((long)t0.s1 * R1 + t1.s1) * R2;
    float v[V];
#pragma unroll
    for (int t = 0; t < V; ++t) {
      const LowresTap t2 = lowres_tap(o2 + t, s.L[2], R2, s.sn[2], s.sl[2]);
      const double a00 = lowres_mix((double)p00[t2.s0], t2.w0, (double)p00[t2.s1], t2.w1);
      const double a01 = lowres_mix((double)p01[t2.s0], t2.w0, (double)p01[t2.s1], t2.w1);
      const double a10 = lowres_mix((double)p10[t2.s0], t2.w0, (double)p10[t2.s1], t2.w1);
      const double a11 = lowres_mix((double)p11[t2.s0], t2.w0, (double)p11[t2.s1], t2.w1);
      const double c0 = lowres_mix(a00, t1.w0, a01, t1.w1);
      const double c1 = lowres_mix(a10, t1.w0, a11, t1.w1);
      v[t] = (float)lowres_mix(c0, t0.w0, c1, t0.w1);
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(y + (long)q * 4) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      y[q] = v[0];
    }
  }
}

// the way back: src -> dst for the samples that drew low resolution, the others are not touched.  grid (x, B), 256 threads; V = 4: per % 4
// == 0 and both are 16-byte aligned.
template <int V>
__global__ __launch_bounds__(kIntensityThreads) void intensity_lowres_copy_kernel(LowresBatch lb, const float* __restrict__ src,
                                                                                  float* __restrict__ dst, unsigned per) {
  static_assert(V == 1 || V == 4, "4 or 16 bytes per thread");
  const int b = blockIdx.y;
  if (!lb.s[b].on) return;
  const float* __restrict__ x = src + (long)b * per;
  float* __restrict__ y = dst + (long)b * per;
  const unsigned groups = per / V;
  for (unsigned q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(y + (long)q * 4) = *reinterpret_cast<const float4*>(x + (long)q * 4);
    } else {
      y[q] = x[q];
    }
  }
}

struct IntensityFlags {
  int on[kFeedMaxBatch];
};

// Statistics of every flagged sample, first half.  grid (G, B) with G = min(kIntensityStatBlocks, ceil(ceil(per / 4) / 256)) — a function
// of `per` alone —, 256 threads.  The fixed order of the sum: voxel i belongs to slot (i / 4) mod (256 G); every slot adds its voxels in
// increasing i to a double that starts at 0; the 256 slots of a workgroup are then halved seven times, slot t += slot t + d for d = 128,
// 64, ..., 1; intensity_stats_finish_kernel adds the G workgroup sums in index order.  min and max ignore NaN (comparisons).
// ws [B][kIntensityStatBlocks][3] double = {sum, min, max} per workgroup.  vec: the batch is 16-byte aligned and per % 4 == 0.
__global__ __launch_bounds__(kIntensityThreads) void intensity_stats_partial_kernel(IntensityFlags fl, const float* __restrict__ image,
                                                                                    unsigned per, int vec, double* __restrict__ ws) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  __shared__ double ssum[kIntensityThreads];
  __shared__ float smin[kIntensityThreads], smax[kIntensityThreads];
  const int b = blockIdx.y;
  if (!fl.on[b]) return;
  const float* __restrict__ x = image + (long)b * per;
  double acc = 0.0;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  const unsigned groups = (per + 3u) / 4u;                                      // per < 2^31
  for (unsigned q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
    const unsigned first = q * 4u;
    float v[4];
    int cnt = 4;
    if (vec) {
      const float4 f = *reinterpret_cast<const float4*>(x + first);
      v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
      cnt = per - first < 4u ? (int)(per - first) : 4;
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = t < cnt ? x[first + t] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < cnt) {
        acc = acc + (double)v[t];
        mn = v[t] < mn ? v[t] : mn;
        mx = v[t] > mx ? v[t] : mx;
      }
    }
  }
  ssum[threadIdx.x] = acc; smin[threadIdx.x] = mn; smax[threadIdx.x] = mx;
  __syncthreads();
  for (int d = kIntensityThreads / 2; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) {
      ssum[threadIdx.x] = ssum[threadIdx.x] + ssum[threadIdx.x + d];
      smin[threadIdx.x] = smin[threadIdx.x + d] < smin[threadIdx.x] ? smin[threadIdx.x + d] : smin[threadIdx.x];
      smax[threadIdx.x] = smax[threadIdx.x + d] > smax[threadIdx.x] ? smax[threadIdx.x + d] : smax[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* o = ws + ((long)b * kIntensityStatBlocks + blockIdx.x) * 3;
    o[0] = ssum[0]; o[1] = (double)smin[0]; o[2] = (double)smax[0];
  }
}

// second half: grid (1), 64 threads, thread b finishes sample b.  stats [B][4] fp32 = {min, max, mean, 0}; the row of a sample that is not
// flagged is left as it is.
__global__ __launch_bounds__(64) void intensity_stats_finish_kernel(IntensityFlags fl, const double* __restrict__ ws, int batch, int blocks,
                                                                    unsigned per, float* __restrict__ stats) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int b = threadIdx.x;
  if (b >= batch || !fl.on[b]) return;
  const double* p = ws + (long)b * kIntensityStatBlocks * 3;
  double sum = p[0], mn = p[1], mx = p[2];
  for (int g = 1; g < blocks; ++g) {
    sum = sum + p[3 * g];
    mn = p[3 * g + 1] < mn ? p[3 * g + 1] : mn;
    mx = p[3 * g + 2] > mx ? p[3 * g + 2] : mx;
  }
  stats[4 * b] = (float)mn;
  stats[4 * b + 1] = (float)mx;
  stats[4 * b + 2] = (float)(sum / (double)per);
  stats[4 * b + 3] = 0.f;
}

struct PointSample {
  int contrast, gamma, invert;      // flags; invert is read only with gamma
  float f;                          // contrast factor
  double g;                         // gamma
};
struct PointBatch {
  PointSample s[kFeedMaxBatch];     // 24 B a record
};

__device__ __forceinline__ float intensity_contrast(float x, float mean, float f, float mn, float mx) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float d = x - mean;
  d = d * f;
  d = d + mean;
  d = d < mn ? mn : d;
  d = d > mx ? mx : d;
  return d;
}

struct GammaConsts {
  double lo, range, den, g;
  int invert;
};

__device__ __forceinline__ float intensity_gamma(float x, const GammaConsts& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float v = c.invert ? -x : x;
  const double t = ((double)v - c.lo) / c.den;
  const double p = c.g == 1.0 ? t : pow(t, c.g);
  const float a = (float)(p * c.range);
  const float y = (float)((double)a + c.lo);
  return c.invert ? -y : y;
}

// contrast and gamma, pointwise and in place.  grid (x, B), 256 threads; V as in intensity_noise_kernel.  stats [B][4] as
// intensity_stats_finish_kernel left it on the same stream, read at a wave-uniform address.  No LDS.
template <int V>
__global__ __launch_bounds__(kIntensityThreads) void intensity_point_kernel(PointBatch pb, const float* __restrict__ stats,
                                                                            float* __restrict__ image, unsigned per) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  static_assert(V == 1 || V == 4, "one voxel or one quad per thread");
  const int b = blockIdx.y;
  const PointSample& s = pb.s[b];
  if (!s.contrast && !s.gamma) return;
  const float mn = stats[4 * b], mx = stats[4 * b + 1], mean = stats[4 * b + 2];
  float lo = mn, hi = mx;                                                       // the extremes behind contrast: the images of min and max
  if (s.contrast) {
    lo = intensity_contrast(mn, mean, s.f, mn, mx);
    hi = intensity_contrast(mx, mean, s.f, mn, mx);
  }
  if (s.invert) {
    const float t = lo;
    lo = -hi;
    hi = -t;
  }
  GammaConsts gc;
  gc.lo = (double)lo;
  gc.range = (double)hi - (double)lo;
  gc.den = gc.range + 1e-7;
  gc.g = s.g;
  gc.invert = s.invert;
  float* __restrict__ x = image + (long)b * per;
  const unsigned groups = per / V;
  for (unsigned q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
    float v[V];
    if constexpr (V == 4) {
      const float4 f = *reinterpret_cast<const float4*>(x + (long)q * 4);
      v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
      v[0] = x[q];
    }
#pragma unroll
    for (int t = 0; t < V; ++t) {
      if (s.contrast) v[t] = intensity_contrast(v[t], mean, s.f, mn, mx);
      if (s.gamma) v[t] = intensity_gamma(v[t], gc);
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(x + (long)q * 4) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      x[q] = v[0];
    }
  }
}

}  // namespace icl
