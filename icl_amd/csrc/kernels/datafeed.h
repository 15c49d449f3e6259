// datafeed.h — on-device training augmentation of the 3-D trainers: RandomRotFlip -> RandomCrop -> ToTensor
// (/root/reference/code/dataloaders/brats2019.py:80-147,177-189; composed at train_inherent_consistent_unet_3D_BraTS.py:66-73)
// as ONE gather kernel over volumes that stay resident in HBM (the whole BraTS2019 training set is 9 GB of fp32; 288 GB per GPU).
// The host draws the random parameters with the reference's numpy call sequence; the kernel maps every output voxel back through
// crop offset -> zero padding -> flip -> rot90 and reads it from the source volume.  The depth axis (fastest) is untouched by
// rot90 / flip (they act on axes 0, 1), so reads and writes are coalesced along it.
#pragma once

namespace icl {

constexpr int kFeedMaxBatch = 16;

struct FeedSample {
  const float* image;        // [n0][n1][n2] fp32
  const uint8_t* label;      // [n0][n1][n2] uint8
  int n0, n1, n2;            // source extents
  int k;                     // np.rot90(., k) on axes (0, 1), k in 0..3
  int flip_axis;             // np.flip axis: 0 or 1; -1 = none
  int p0, p1, p2;            // zero padding added on both sides of each axis (RandomCrop pads small volumes)
  int c0, c1, c2;            // crop origin in the padded, rotated, flipped volume
};

struct FeedBatch {
  FeedSample s[kFeedMaxBatch];
};

// np.rot90(x, k) on axes (0, 1) of an array x of extents e0 x e1, read backwards: rotated[a][c] = x[sa][sc].  Every gather of this
// header uses it: the crop and slice kernels with the source extents n0, n1, the volume kernels with the patch extents R0, R1.
__device__ __forceinline__ void rot90_source(int k, int a, int c, int e0, int e1, int& sa, int& sc) {
  switch (k & 3) {
    case 0: sa = a; sc = c; break;
    case 1: sa = c; sc = e1 - 1 - a; break;
    case 2: sa = e0 - 1 - a; sc = e1 - 1 - c; break;
    default: sa = e0 - 1 - c; sc = a; break;
  }
}

// The crop chain's map into the source, stated once: Y = flip(rot90(x, k), flip_axis) is the rotated and flipped volume of extents
// (r0, r1, n2), r0 and r1 being n0 and n1 swapped for odd k; this is the source offset of its voxel (a, c, 0).  The map is affine in
// (a, c): an origin and one SIGNED source stride for each of the axes 0 and 1, and stride 1 along depth.
__device__ __forceinline__ long crop_feed_row(const FeedSample& s, int r0, int r1, int a, int c) {
  if (s.flip_axis == 0) a = r0 - 1 - a;
  else if (s.flip_axis == 1) c = r1 - 1 - c;
  int sa, sc;
  rot90_source(s.k, a, c, s.n0, s.n1, sa, sc);
  return ((long)sa * s.n1 + sc) * s.n2;
}

// V labels (0..255) as int64 at p; V = 4: p is 16-byte aligned, two 16-byte stores whose high dwords are 0
template <int V>
__device__ __forceinline__ void feed_store_labels(long long* p, const unsigned (&lab)[V]) {
  if constexpr (V == 4) {
    uint4* lp = reinterpret_cast<uint4*>(p);
    lp[0] = make_uint4(lab[0], 0u, lab[1], 0u);
    lp[1] = make_uint4(lab[2], 0u, lab[3], 0u);
  } else {
    p[0] = (long long)lab[0];
  }
}

// V image voxels at `image` (V = 4: one 16-byte store to a 16-byte aligned address) and their labels at `label`
template <int V>
__device__ __forceinline__ void feed_store(float* image, long long* label, const float (&v)[V], const unsigned (&lab)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(image) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    image[0] = v[0];
  }
  feed_store_labels<V>(label, lab);
}

// image_out [B][1][o0][o1][o2] fp32, label_out [B][o0][o1][o2] int64.  grid (ceil(o2/64)... flat), one thread per output voxel.
__global__ __launch_bounds__(256) void crop_rotflip_kernel(FeedBatch fb, float* __restrict__ image_out, long long* __restrict__ label_out, int B,
                                                           int o0, int o1, int o2) {
  const long per = (long)o0 * o1 * o2, total = per * B;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int b = (int)(e / per);
    long r = e % per;
    const int l = (int)(r % o2);
    r /= o2;
    const int j = (int)(r % o1), i = (int)(r / o1);
    const FeedSample& s = fb.s[b];
    // extents after rot90: odd k swaps axes 0 and 1
    const int r0 = (s.k & 1) ? s.n1 : s.n0, r1 = (s.k & 1) ? s.n0 : s.n1;
    // crop -> padded coordinates -> unpadded (rotated + flipped) coordinates
    const int a = s.c0 + i - s.p0, c = s.c1 + j - s.p1, d = s.c2 + l - s.p2;
    float v = 0.f;
    long long lab = 0;
    if (a >= 0 && a < r0 && c >= 0 && c < r1 && d >= 0 && d < s.n2) {
      const long src = crop_feed_row(s, r0, r1, a, c) + d;
      v = s.image[src];
      lab = (long long)s.label[src];
    }
    image_out[e] = v;
    label_out[e] = lab;
  }
}

// ---- multi-modal volumes: the chain of crop_rotflip_kernel on images [C][n0][n1][n2] (co-registered channels, BraTS's four MR
// modalities) with ONE label [n0][n1][n2].  The map output voxel -> crop -> padding -> flip -> rot90 -> source index does not depend on
// the channel, so it is computed once per output position and used for all C channels (channel stride n0 * n1 * n2) and for the
// label, which is read and written once.
//
// The integer gather of that chain, the only one of crop_rotflip_channels_kernel and the path of a sample without the affine stage in
// crop_rotflip_affine_kernel: V consecutive output depth voxels from (i, j, l) on, for all C channels, stored at `img` (channel stride
// `vox`) and `lab`, which point at the output voxel.  V = 4: the store is always a quad per channel and feed_store_labels; the load is
// a quad where the four sources lie inside the row at a 16-byte aligned address, four guarded scalar loads otherwise (the scheme of
// window_gather_kernel<4>).  The values are copied, never computed with.
template <int V>
__device__ __forceinline__ void crop_feed_gather(const FeedSample& s, int r0, int r1, int C, int i, int j, int l, float* __restrict__ img, long vox,
                                                 long long* __restrict__ lab) {
  const long cs = (long)s.n0 * s.n1 * s.n2;                                   // channel stride of the source
  // crop -> padded coordinates -> unpadded (rotated + flipped) coordinates
  const int a = s.c0 + i - s.p0, c = s.c1 + j - s.p1, d = s.c2 + l - s.p2;
  const bool row = a >= 0 && a < r0 && c >= 0 && c < r1;
  const long base = row ? crop_feed_row(s, r0, r1, a, c) : 0;
  bool in[V];
  unsigned lv[V];
#pragma unroll
  for (int t = 0; t < V; ++t) {
    in[t] = row && d + t >= 0 && d + t < s.n2;
    lv[t] = in[t] ? (unsigned)s.label[base + d + t] : 0u;
  }
  const bool inside = V == 4 && row && d >= 0 && d + V <= s.n2;               // the whole quad lies in the row
  for (int ch = 0; ch < C; ++ch) {
    const float* __restrict__ src = s.image + ch * cs + base + d;             // dereferenced only where in[t]
    float v[V];
    if (inside && ((uintptr_t)src & 15) == 0) {
      const float4 f = *reinterpret_cast<const float4*>(src);
      v[0] = f.x;
      if constexpr (V == 4) { v[1] = f.y; v[2] = f.z; v[3] = f.w; }
    } else {
#pragma unroll
      for (int t = 0; t < V; ++t) v[t] = in[t] ? src[t] : 0.f;
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(img + ch * vox) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      img[ch * vox] = v[0];
    }
  }
  feed_store_labels<V>(lab, lv);
}

// image_out [B][C][o0][o1][o2] fp32, label_out [B][o0][o1][o2] int64.  grid (x, B): one sample per blockIdx.y, so its record is
// wave-uniform.  One thread per V consecutive depth voxels (V = 4: o2 % 4 == 0 and both outputs 16-byte aligned).  No LDS, no atomics.
// With C = 1 the result is crop_rotflip_kernel's bit for bit.
template <int V>
__global__ __launch_bounds__(256) void crop_rotflip_channels_kernel(FeedBatch fb, float* __restrict__ image_out, long long* __restrict__ label_out,
                                                                    int C, int o0, int o1, int o2) {
  static_assert(V == 1 || V == 4, "one voxel or one quad per thread");
  const int q2 = o2 / V;
  const unsigned per = (unsigned)o0 * o1 * q2;                                // the launcher keeps o0 * o1 * o2 below 2^31
  const int b = blockIdx.y;
  const FeedSample& s = fb.s[b];
  const long vox = (long)o0 * o1 * o2;                                        // channel stride of the output
  // extents after rot90: odd k swaps axes 0 and 1
  const int r0 = (s.k & 1) ? s.n1 : s.n0, r1 = (s.k & 1) ? s.n0 : s.n1;
  float* __restrict__ img = image_out + (long)b * C * vox;
  long long* __restrict__ lab = label_out + (long)b * vox;
  for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < per; r += gridDim.x * blockDim.x) {
    const int l = (int)(r % q2) * V;
    const unsigned rj = r / q2;
    const long e = (long)r * V;                                               // = (i * o1 + j) * o2 + l
    crop_feed_gather<V>(s, r0, r1, C, (int)(rj / o1), (int)(rj % o1), l, img + e, vox, lab + e);
  }
}

// ---- channel-wise intensity normalisation of a resident volume [C][voxels] (MONAI NormalizeIntensityd(nonzero, channel_wise); the
// reference's itensity_normalize_one_volume): per channel, over the voxels of the mask (kNormNonzero: x != 0, kNormPositive: x > 0,
// kNormAll), count, mean and POPULATION standard deviation in double, two passes: sum and count, then sum of (x - mean)^2 with the mean
// read from `stats`.  No atomics.  The fixed order of every sum (that of intensity_stats_partial_kernel): voxel i belongs to slot (i / 4)
// mod (256 G), G = gridDim.x a function of `voxels` alone; every slot adds its voxels in increasing i to a double that starts at 0; the
// 256 slots of a workgroup are halved eight times, slot t += slot t + d for d = 128, 64, ..., 1; channel_norm_finish_kernel adds the
// G workgroup sums in index order.  stats [C][4] double = {count, mean, std, 0}; an empty mask gives {0, 0, 0, 0}.
constexpr int kChannelNormThreads = 256;
constexpr int kChannelNormBlocks = 256;      // most workgroups per channel: ws holds [C][kChannelNormBlocks][2] doubles
constexpr int kChannelNormMaxChannels = 16;
enum ChannelNormMask { kNormNonzero = 0, kNormPositive = 1, kNormAll = 2 };

__device__ __forceinline__ bool channel_norm_in_mask(float x, int mask_mode) {
  return mask_mode == kNormAll || (mask_mode == kNormPositive ? x > 0.f : x != 0.f);
}

// grid (G, C), 256 threads.  PASS 1: ws[c][g] = {sum of x, count}.  PASS 2: ws[c][g] = {sum of (x - mean_c)^2, count}, mean_c = stats[4 c + 1].
// vec: the volume is 16-byte aligned and voxels % 4 == 0, so every group of every channel is one 16-byte load.
template <int PASS>
__global__ __launch_bounds__(kChannelNormThreads) void channel_norm_partial_kernel(const float* __restrict__ image, long voxels, int mask_mode, int vec,
                                                                                   const double* __restrict__ stats, double* __restrict__ ws) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  __shared__ double ssum[kChannelNormThreads], scnt[kChannelNormThreads];
  const int ch = blockIdx.y;
  const float* __restrict__ x = image + (long)ch * voxels;
  double mean = 0.0;
  if constexpr (PASS == 2) mean = stats[4 * ch + 1];
  double acc = 0.0, cnt = 0.0;
  const unsigned groups = (unsigned)((voxels + 3) / 4);                       // the launcher keeps voxels below 2^31
  for (unsigned q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
    const long first = (long)q * 4;
    float v[4];
    int n = 4;
    if (vec) {
      const float4 f = *reinterpret_cast<const float4*>(x + first);
      v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
      n = voxels - first < 4 ? (int)(voxels - first) : 4;
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = t < n ? x[first + t] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < n && channel_norm_in_mask(v[t], mask_mode)) {
        if constexpr (PASS == 1) {
          acc = acc + (double)v[t];
        } else {
          const double dv = (double)v[t] - mean;
          acc = acc + dv * dv;
        }
        cnt = cnt + 1.0;
      }
    }
  }
  ssum[threadIdx.x] = acc; scnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int d = kChannelNormThreads / 2; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) {
      ssum[threadIdx.x] = ssum[threadIdx.x] + ssum[threadIdx.x + d];
      scnt[threadIdx.x] = scnt[threadIdx.x] + scnt[threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* o = ws + ((long)ch * kChannelNormBlocks + blockIdx.x) * 2;
    o[0] = ssum[0]; o[1] = scnt[0];
  }
}

// grid (1), 64 threads, thread c finishes channel c.  PASS 1: stats[c] = {count, sum / count, 0, 0}.  PASS 2: stats[c][2] = sqrt(sum / count).
// A channel whose mask is empty gets {0, 0, 0, 0}.
template <int PASS>
__global__ __launch_bounds__(64) void channel_norm_finish_kernel(const double* __restrict__ ws, int channels, int blocks, double* __restrict__ stats) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int ch = threadIdx.x;
  if (ch >= channels) return;
  const double* p = ws + (long)ch * kChannelNormBlocks * 2;
  double sum = p[0], cnt = p[1];
  for (int g = 1; g < blocks; ++g) {
    sum = sum + p[2 * g];
    cnt = cnt + p[2 * g + 1];
  }
  double* o = stats + 4 * ch;
  if constexpr (PASS == 1) {
    o[0] = cnt;
    o[1] = cnt > 0.0 ? sum / cnt : 0.0;
    o[2] = 0.0;
    o[3] = 0.0;
  } else {
    o[2] = cnt > 0.0 ? sqrt(sum / cnt) : 0.0;
  }
}

// x <- (x - m) / s in fp32, m = fp32(mean), s = fp32(std) with 0 -> 1: a true subtraction and a true division, each rounded on its own.
// apply_all = 0: only the voxels of the mask change; 1: every voxel.  A channel with an empty mask is left as it is.  grid (x, C).
template <int V>
__global__ __launch_bounds__(kChannelNormThreads) void channel_norm_apply_kernel(float* __restrict__ image, long voxels, int mask_mode, int apply_all,
                                                                                 const double* __restrict__ stats) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  static_assert(V == 1 || V == 4, "4 or 16 bytes per thread");
  const int ch = blockIdx.y;
  const double* st = stats + 4 * ch;
  if (!(st[0] > 0.0)) return;
  const float m = (float)st[1];
  float sd = (float)st[2];
  if (sd == 0.f) sd = 1.f;
  float* __restrict__ x = image + (long)ch * voxels;
  const unsigned groups = (unsigned)(voxels / V);
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
      if (apply_all || channel_norm_in_mask(v[t], mask_mode)) {
        const float dv = v[t] - m;
        v[t] = dv / sd;
      }
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(x + (long)q * 4) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      x[q] = v[0];
    }
  }
}

// ---- 2-D trainers: RandomGenerator (dataloaders/dataset.py:147-166 of the reference) as ONE gather over slices resident in HBM.
// The reference chain is "maybe rot90 + flip, else maybe ndimage.rotate by an integer angle, then ndimage.zoom to the patch", all
// order 0.  Two nearest-neighbour samplings compose into one gather: the zoom maps the output pixel to an INTEGER pixel (a, b) of
// the intermediate image, and rot90 / flip / rotate map (a, b) to the stored slice.  Every coordinate is formed in fp64 with the
// products and sums scipy's C code performs, each rounded on its own (hipcc contracts a * b + c into an fma by default, scipy
// does not: `fp contract(off)` below), so the result equals the reference bit for bit, zero edges included:
//   zoom, per axis:  c = (double)i * z, z = (n_in - 1) / (n_out - 1);  c < 0 or c > n_in - 1 -> 0 (mode='constant': in double
//                    (n_out - 1) * z can land just ABOVE n_in - 1, and scipy then writes a zero last row / column); else floor(c + 0.5)
//   rotate:          c0 = (off0 + a * M00) + b * M01, c1 = (off1 + a * M10) + b * M11;  outside [0, n - 1] -> 0; else floor(c + 0.5)
constexpr int kSliceMaxBatch = 32;
enum SliceBranch { kSliceNone = 0, kSliceRotFlip = 1, kSliceRotate = 2 };

struct SliceSample {
  const float* image;        // [n0][n1] fp32
  const uint8_t* label;      // [n0][n1] uint8
  int n0, n1;                // source extents
  int branch;                // SliceBranch
  int k, flip_axis;          // kSliceRotFlip: np.flip(np.rot90(x, k), flip_axis)
  int pad_;
  double m00, m01, m10, m11; // kSliceRotate: [[cos, sin], [-sin, cos]] of the angle ...
  double off0, off1;         // ... and centre - M @ centre, computed on the host in double
  double z0, z1;             // zoom factors (r - 1) / (o - 1) of the extents r AFTER rot90 (odd k swaps them)
};

struct SliceBatch {
  SliceSample s[kSliceMaxBatch];     // 104 B a record: 3,328 B of the 4 KB kernel-argument block
};

// zoom of one axis (scipy NI_ZoomShift, order 0, mode 'constant'): source index of output index i, -1 = the output is 0
__device__ __forceinline__ int slice_zoom_index(int i, double z, int n_in) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double c = (double)i * z;
  if (!(c >= 0.0 && c <= (double)(n_in - 1))) return -1;
  return (int)floor(c + 0.5);
}

// image_out [B][1][o0][o1] fp32, label_out [B][o0][o1] uint8; one thread per output pixel, o1 fastest (coalesced writes)
__global__ __launch_bounds__(256) void slice_augment_kernel(SliceBatch sb, float* __restrict__ image_out, uint8_t* __restrict__ label_out, int B,
                                                            int o0, int o1) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const long per = (long)o0 * o1, total = per * B;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int b = (int)(e / per);
    const int r = (int)(e % per);
    const int i = r / o1, j = r % o1;
    const SliceSample& s = sb.s[b];
    const bool swap = s.branch == kSliceRotFlip && (s.k & 1);
    const int r0 = swap ? s.n1 : s.n0, r1 = swap ? s.n0 : s.n1;
    int a = slice_zoom_index(i, s.z0, r0), c = slice_zoom_index(j, s.z1, r1);
    int sa = -1, sc = -1;
    if (a >= 0 && c >= 0) {
      if (s.branch == kSliceRotFlip) {
        if (s.flip_axis == 0) a = r0 - 1 - a;
        else c = r1 - 1 - c;
        rot90_source(s.k, a, c, s.n0, s.n1, sa, sc);
      } else if (s.branch == kSliceRotate) {
        const double da = (double)a, dc = (double)c;
        const double p00 = da * s.m00, p01 = dc * s.m01, p10 = da * s.m10, p11 = dc * s.m11;
        const double c0 = (s.off0 + p00) + p01;
        const double c1 = (s.off1 + p10) + p11;
        if (c0 >= 0.0 && c0 <= (double)(s.n0 - 1) && c1 >= 0.0 && c1 <= (double)(s.n1 - 1)) {
          sa = (int)floor(c0 + 0.5);
          sc = (int)floor(c1 + 0.5);
        }
      } else {
        sa = a; sc = c;
      }
    }
    float v = 0.f;
    uint8_t lab = 0;
    if (sa >= 0) {
      const long src = (long)sa * s.n1 + sc;
      v = s.image[src];
      lab = s.label[src];
    }
    image_out[e] = v;
    label_out[e] = lab;
  }
}

// Plain batched ndimage.zoom(order=0) of B slices [n0][n1] -> [o0][o1] that share one extent: both resizes of the 2-D validation loop
// (val_2D.py:41,48 of the reference; T = float for the slices going in, long long for the arg-max maps going back).
template <typename T>
__global__ __launch_bounds__(256) void slice_resize_kernel(const T* __restrict__ src, T* __restrict__ dst, int B, int n0, int n1, int o0, int o1,
                                                           double z0, double z1) {
  const long per = (long)o0 * o1, total = per * B;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long b = e / per;
    const int r = (int)(e % per);
    const int a = slice_zoom_index(r / o1, z0, n0), c = slice_zoom_index(r % o1, z1, n1);
    dst[e] = (a >= 0 && c >= 0) ? src[(b * n0 + a) * n1 + c] : T(0);
  }
}

// ---- 3-D AMOS trainer: the random transforms of train_inherent_consistent_unet_3D_AMOS22.py:102-133 (RandSpatialCropd ->
// SpatialPadd -> three RandFlipd -> RandRotate90d -> RandShiftIntensityd) as ONE gather over volumes resident in HBM.  The chain
// differs from crop_rotflip_kernel's (symmetric padding AFTER the crop, three independent flips with the depth axis among them,
// an intensity term that also lands on the padded voxels), so it has a kernel of its own.  Forward, per sample:
//   x = src[c : c + s];  x = zero-pad to R with l_a on the left;  flip axis 0 / 1 / 2 for bits 0 / 1 / 2 of `flip`;
//   x = np.rot90(x, k, axes=(0, 1));  image only: fp32(fp32(x * mul) + add) on EVERY voxel.
// Every output voxel is mapped backwards through rot90 -> flips -> padding -> crop origin (volume_feed_gather).  Odd k needs
// R0 == R1 (the launcher checks), so the flipped patch always has the output's extents.
struct VolumeFeedSample {
  const float* image;        // [n0][n1][n2] fp32
  const uint8_t* label;      // [n0][n1][n2] uint8
  int n1, n2;                // source extents of axes 1 and 2 (the launcher has checked c + s <= n on every axis)
  int c0, c1, c2;            // crop origin in the source (DEV: the largest legal origin, n - s)
  int s0, s1, s2;            // crop size, min(R, n) per axis
  int l0, l1, l2;            // zero padding on the left of each axis (R - s - l on the right)
  int flip;                  // bit a: np.flip on axis a
  int k;                     // np.rot90(., k, axes=(0, 1)), k in 0..3
  float mul, add;            // intensity: v * mul + add
};

struct VolumeFeedBatch {
  VolumeFeedSample s[kFeedMaxBatch];     // 80 B a record: 1,280 B of the 4 KB kernel-argument block
};

// The crop origin of sample b from device memory (DEV kernels): origins [B][3] int32, as rank_select_kernel (rankindex.h) left it on
// the same stream, read once per workgroup at a wave-uniform address.  On entry c0, c1, c2 hold the LARGEST legal origin n - s (the
// launcher put it in the record); an origin outside [0, n - s] is clamped into it, so no content of that buffer can send a read
// outside the volume.
__device__ __forceinline__ void clamp_device_origin(const int* __restrict__ origins, int b, int& c0, int& c1, int& c2) {
  const int* __restrict__ o = origins + 3 * b;
  c0 = o[0] < 0 ? 0 : (o[0] > c0 ? c0 : o[0]);
  c1 = o[1] < 0 ? 0 : (o[1] > c1 ? c1 : o[1]);
  c2 = o[2] < 0 ? 0 : (o[2] > c2 ? c2 : o[2]);
}

// The integer gather, the only one of volume_feed_kernel and the path of a sample without the affine stage in
// volume_feed_affine_kernel: V consecutive output depth voxels from l on, at the flipped patch coordinates (fa, fc) of axes 0, 1.
// Padded -> cropped coordinates -> source at the crop origin (c0, c1, c2); the source is walked forwards or, with flip bit 2,
// backwards along depth; a voxel of the padding is 0 with label 0; then fp32(fp32(x * mul) + add) on EVERY voxel (two roundings:
// the pragma is repeated here because it binds to the compound statement it stands in, not to the caller's).
template <int V>
__device__ __forceinline__ void volume_feed_gather(const VolumeFeedSample& s, int c0, int c1, int c2, int fa, int fc, int l, int R2,
                                                   float (&v)[V], unsigned (&lab)[V]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int a = fa - s.l0, c = fc - s.l1;
  const bool rev = (s.flip & 4) != 0;
  const int d0 = (rev ? R2 - 1 - l : l) - s.l2, step = rev ? -1 : 1;
  const bool row = a >= 0 && a < s.s0 && c >= 0 && c < s.s1;
  const long base = row ? ((long)(c0 + a) * s.n1 + (c1 + c)) * s.n2 + c2 : 0;
#pragma unroll
  for (int t = 0; t < V; ++t) {
    const int d = d0 + t * step;
    float x = 0.f;
    lab[t] = 0u;
    if (row && d >= 0 && d < s.s2) {
      x = s.image[base + d];
      lab[t] = s.label[base + d];
    }
    const float m = x * s.mul;
    v[t] = m + s.add;
  }
}

// image_out [B][1][R0][R1][R2] fp32, label_out [B][R0][R1][R2] int64.  grid (x, B).  One thread per V consecutive depth voxels (V = 4:
// R2 % 4 == 0, both outputs 16-byte aligned).  No LDS, no atomics.  DEV = false (icl_volume_feed): the crop origin is the record's c0,
// c1, c2 and `origins` is not read.  DEV = true (icl_volume_feed_origins): clamp_device_origin.
template <int V, bool DEV>
__global__ __launch_bounds__(256) void volume_feed_kernel(VolumeFeedBatch fb, const int* __restrict__ origins, float* __restrict__ image_out,
                                                          long long* __restrict__ label_out, int R0, int R1, int R2) {
  static_assert(V == 1 || V == 4, "one voxel or one quad per thread");
  const int q2 = R2 / V;
  const unsigned per = (unsigned)R0 * R1 * q2;                                // the launcher keeps R0 * R1 * R2 below 2^31
  const int b = blockIdx.y;                                                   // one sample per grid row: its record is wave-uniform
  const VolumeFeedSample& s = fb.s[b];
  int c0 = s.c0, c1 = s.c1, c2 = s.c2;
  if constexpr (DEV) clamp_device_origin(origins, b, c0, c1, c2);
  for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < per; r += gridDim.x * blockDim.x) {
    const long e = (long)b * per + r;
    const int l = (int)(r % q2) * V;
    const unsigned rj = r / q2;
    const int j = (int)(rj % R1), i = (int)(rj / R1);
    int fa, fc;                                                               // out[i][j] = flipped[fa][fc]
    rot90_source(s.k, i, j, R0, R1, fa, fc);
    if (s.flip & 1) fa = R0 - 1 - fa;
    if (s.flip & 2) fc = R1 - 1 - fc;
    float v[V];
    unsigned lab[V];
    volume_feed_gather<V>(s, c0, c1, c2, fa, fc, l, R2, v, lab);
    feed_store<V>(image_out + e * V, label_out + e * V, v, lab);
  }
}

// ---- the AFFINE stage of both 3-D chains (MONAI RandAffined, nnU-Net's rotation and scaling): one trilinear sampler about the patch
// centre, used by volume_feed_affine_kernel (AMOS) and crop_rotflip_affine_kernel (BraTS).  The definition is in DESIGN.md §2 "Affine
// stage of the 3-D feed"; tests/affine_feed_ref.py and tests/crop_affine_ref.py restate it in numpy.  For the integer patch coordinates
// p of a voxel, every fp64 product and sum rounded on its own,
//   u_a = p_a - (R_a - 1) / 2,  t_a = (c_a - pad_a) + (R_a - 1) / 2              (both exact),
//   x_a = t_a + ((M_a0 u_0 + M_a1 u_1) + M_a2 u_2)                               (a coordinate of the WHOLE sampled volume, not of the crop),
//   image: i_a = floor(x_a), f_a = x_a - i_a; the eight taps in the order (0,0,0), (0,0,1), ..., (1,1,1), a tap outside [0, n_a - 1]
//          on any axis counting as 0; sum of double(tap) * ((w_0 w_1) w_2), w_a = f_a for bit 1 and 1 - f_a for bit 0, left to right
//          in double, rounded once to fp32;
//   label: the voxel at rint(x_a) per axis (half to even); 0 when a rounded index is outside [0, n_a - 1].
// Every range test is made on the DOUBLE, before any conversion to int, so no M and no content of a device buffer can send a read outside
// the volume (the launchers bound |M_ab| by 16 all the same, which keeps |x| far below 2^31).  The definition is per voxel, so the result
// does not depend on how threads are mapped to voxels.  Each function repeats the pragma: it binds to the compound statement it stands in.

// The sampled volume: extents, and the element offset of its voxel (a, c, d) = origin + a * stride0 + c * stride1 + d (signed strides)
struct AffineVolume {
  int n0, n1, n2;
  long origin, stride0, stride1;
};

// what the voxels of a sample share: the doubled half extents 2 h_a = R_a - 1, and t_a = (c_a - pad_a) + h_a
struct AffineFrame {
  int hh0, hh1, hh2;
  double t0, t1, t2;
};

__device__ __forceinline__ AffineFrame affine_frame(int R0, int R1, int R2, int d0, int d1, int d2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  AffineFrame f;
  f.hh0 = R0 - 1; f.hh1 = R1 - 1; f.hh2 = R2 - 1;
  f.t0 = (double)d0 + (double)f.hh0 * 0.5; f.t1 = (double)d1 + (double)f.hh1 * 0.5; f.t2 = (double)d2 + (double)f.hh2 * 0.5;
  return f;
}

// One axis of one voxel.  j0, j1: an index INSIDE [0, n - 1] for each of the two taps floor(x), floor(x) + 1: its own where its range
// test let it in, else the other tap's, else 0 (n >= 1), so every tap has an address inside the volume whatever x is.
struct AffineAxis {
  double w0, w1;             // 1 - f, f
  int j0, j1;
  unsigned in;               // bit 0: tap floor(x) lies in [0, n - 1]; bit 1: tap floor(x) + 1 does
  int nn;                    // rint(x), or -1 outside [0, n - 1]
};

__device__ __forceinline__ AffineAxis affine_axis(double x, int n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double top = (double)(n - 1);
  const double fl = floor(x);
  const double f = x - fl;
  const bool in0 = fl >= 0.0 && fl <= top;            // on the double: a NaN or a huge x fails both
  const bool in1 = fl >= -1.0 && fl <= top - 1.0;
  const int i0 = (in0 || in1) ? (int)fl : 0;          // -1 .. n - 1
  AffineAxis a;
  a.j0 = in0 ? i0 : 0;                                // in1 alone: floor(x) = -1, and the other tap is 0
  a.j1 = in1 ? i0 + 1 : a.j0;                         // in0 alone: floor(x) = n - 1 = j0
  a.in = (in0 ? 1u : 0u) | (in1 ? 2u : 0u);
  a.w0 = 1.0 - f;
  a.w1 = f;
  const double rn = rint(x);                          // half to even
  a.nn = (rn >= 0.0 && rn <= top) ? (int)rn : -1;
  return a;
}

// The taps of one voxel, from the definition ONCE for all channels.  Every tap has an address inside the volume (affine_axis), so the
// loads need no branch and are in flight together; the value of a tap outside is replaced by 0 after the load (affine_value).
struct AffineTaps {
  long row[4];               // offsets of the taps (0,0,0), (0,1,0), (1,0,0), (1,1,0)
  int step;                  // 0 or 1: from tap (., ., 0) to tap (., ., 1)
  unsigned in;               // bit (4 b0 + 2 b1 + b2): tap (b0, b1, b2) is inside the volume
  double w[8];               // (w_0 w_1) w_2 of tap (4 b0 + 2 b1 + b2)
  long label;                // offset of the label's voxel; voxel (0, 0, 0) stands in where `labelled` is 0
  unsigned labelled;         // 1: every rounded index is inside; 0: the label is 0
};

__device__ __forceinline__ AffineTaps affine_taps(int p0, int p1, int p2, const double (&m)[9], const AffineFrame& f, const AffineVolume& vol) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  // u_a = p_a - h_a as (2 p_a - 2 h_a) / 2: an integer halved, exact like the difference
  const double u0 = (double)(2 * p0 - f.hh0) * 0.5, u1 = (double)(2 * p1 - f.hh1) * 0.5, u2 = (double)(2 * p2 - f.hh2) * 0.5;
  const AffineAxis a0 = affine_axis(f.t0 + ((m[0] * u0 + m[1] * u1) + m[2] * u2), vol.n0);      // every product and sum
  const AffineAxis a1 = affine_axis(f.t1 + ((m[3] * u0 + m[4] * u1) + m[5] * u2), vol.n1);      // rounded on its own
  const AffineAxis a2 = affine_axis(f.t2 + ((m[6] * u0 + m[7] * u1) + m[8] * u2), vol.n2);      // (contraction off)
  AffineTaps t;
  const long ra0 = vol.origin + (long)a0.j0 * vol.stride0, ra1 = vol.origin + (long)a0.j1 * vol.stride0;
  const long rc0 = (long)a1.j0 * vol.stride1 + a2.j0, rc1 = (long)a1.j1 * vol.stride1 + a2.j0;
  t.row[0] = ra0 + rc0; t.row[1] = ra0 + rc1; t.row[2] = ra1 + rc0; t.row[3] = ra1 + rc1;
  t.step = a2.j1 - a2.j0;
  // The product of the three axes' bits, in integer arithmetic throughout: a flag kept as a lane mask costs a scalar register pair.
  const unsigned in01 = ((0u - (a0.in & 1u)) & a1.in) | (((0u - (a0.in >> 1)) & a1.in) << 2);        // bit (2 b0 + b1)
  t.in = ((0u - (in01 & 1u)) & a2.in) | (((0u - ((in01 >> 1) & 1u)) & a2.in) << 2) |
         (((0u - ((in01 >> 2) & 1u)) & a2.in) << 4) | (((0u - (in01 >> 3)) & a2.in) << 6);
  const double w00 = a0.w0 * a1.w0, w01 = a0.w0 * a1.w1, w10 = a0.w1 * a1.w0, w11 = a0.w1 * a1.w1;
  t.w[0] = w00 * a2.w0; t.w[1] = w00 * a2.w1; t.w[2] = w01 * a2.w0; t.w[3] = w01 * a2.w1;
  t.w[4] = w10 * a2.w0; t.w[5] = w10 * a2.w1; t.w[6] = w11 * a2.w0; t.w[7] = w11 * a2.w1;
  const int lin = (a0.nn | a1.nn | a2.nn) >= 0 ? 1 : 0;
  t.labelled = (unsigned)lin;
  t.label = vol.origin + (long)(a0.nn * lin) * vol.stride0 + (long)(a1.nn * lin) * vol.stride1 + a2.nn * lin;
  return t;
}

// The value of one channel `p` at the taps: eight unconditional fp32 loads; bit k of `in` becomes an all-ones or all-zeros word that
// tap k is ANDed with (a select without a compare: a tap inside keeps every bit, a NaN its payload; a tap outside becomes +0); then
// the eight-term sum, left to right in double, rounded once.
__device__ __forceinline__ float affine_value(const float* __restrict__ p, const AffineTaps& t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float y[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) y[k] = p[t.row[k >> 1] + (k & 1) * t.step];
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double term = (double)__uint_as_float(__float_as_uint(y[k]) & (0u - ((t.in >> k) & 1u))) * t.w[k];
    acc = k == 0 ? term : acc + term;
  }
  return (float)acc;
}

// The output voxel (i, j, l) of thread e of an affine sample, one thread per voxel.  Where R1 % 8 == 0 and R2 % 8 == 0 a wave (64
// consecutive e) takes a compact 8 x 8 tile of (rows, depth): rows j .. j + 7, depth l .. l + 7, whose taps touch fewer cache lines
// under rotation than those of 64 voxels in a line (it writes eight runs of 32 B a channel); otherwise 64 consecutive voxels.
// Measured on crop_rotflip_affine_kernel at 2 x 4 x 96^3 under rotation (profiles/crop_affine.md): one quad per thread with guarded
// loads 266 us, one voxel per thread 122 us, with loads that need no branch 80 us, in tiles 71 us.
__device__ __forceinline__ void affine_thread_voxel(unsigned e, int R1, int R2, int& i, int& j, int& l) {
  if ((R1 & 7) == 0 && (R2 & 7) == 0) {
    const unsigned tiles2 = (unsigned)R2 >> 3, tiles1 = (unsigned)R1 >> 3;
    const unsigned tile = e >> 6, lane = e & 63u;
    l = (int)((tile % tiles2) << 3 | (lane & 7u));
    const unsigned tj = tile / tiles2;
    j = (int)((tj % tiles1) << 3 | (lane >> 3));
    i = (int)(tj / tiles1);
  } else {
    l = (int)(e % R2);
    const unsigned rj = e / R2;
    j = (int)(rj % R1);
    i = (int)(rj / R1);
  }
}

// ---- the AMOS chain with the stage between the pad and the flips: crop -> symmetric pad -> affine about the patch centre -> flips ->
// rot90 -> intensity.  A sample either has the stage (`affine` = 1) or it does not: without it the sample goes through
// volume_feed_gather, as in volume_feed_kernel.  With it, the output voxel is mapped back through rot90 and the flips to integer patch
// coordinates p as there, the sampler reads the whole source volume (strides n1 n2 and n2), and fp32(fp32(v * mul) + add) follows.
struct VolumeFeedAffineSample {
  VolumeFeedSample f;        // as for volume_feed_kernel
  int n0;                    // source extent of axis 0: the affine gather reads the whole volume
  int affine;                // 1: the sample has the affine stage; 0: m is not read
  double m[9];               // M, row-major
};

struct VolumeFeedAffineBatch {
  VolumeFeedAffineSample s[kFeedMaxBatch];     // 160 B a record: 2,560 B of the 4 KB kernel-argument block
};

// Arguments and stores of volume_feed_kernel<V, DEV>; grid (x, B), one sample per blockIdx.y, so its record and `affine` are
// wave-uniform.  V is the form of the INTEGER path.  An affine sample takes one thread per output voxel in both instances
// (affine_thread_voxel); the launcher sizes the grid for that when the launch has an affine sample, and the threads an integer-path
// sample does not need leave at once.  DEV = true: t_a is formed on the device from the clamped origin (clamp_device_origin).
// No LDS, no atomics.
template <int V, bool DEV>
__global__ __launch_bounds__(256) void volume_feed_affine_kernel(VolumeFeedAffineBatch fb, const int* __restrict__ origins,
                                                                 float* __restrict__ image_out, long long* __restrict__ label_out, int R0, int R1,
                                                                 int R2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  static_assert(V == 1 || V == 4, "one voxel or one quad per thread");
  const unsigned voxels = (unsigned)R0 * R1 * R2;                             // the launcher keeps R0 * R1 * R2 below 2^31
  const int b = blockIdx.y;
  const VolumeFeedAffineSample& rec = fb.s[b];
  const VolumeFeedSample& s = rec.f;
  int c0 = s.c0, c1 = s.c1, c2 = s.c2;
  if constexpr (DEV) clamp_device_origin(origins, b, c0, c1, c2);
  float* __restrict__ img = image_out + (long)b * voxels;
  long long* __restrict__ lab = label_out + (long)b * voxels;
  if (!rec.affine) {
    const int q2 = R2 / V;
    for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < voxels / V; r += gridDim.x * blockDim.x) {
      const int l = (int)(r % q2) * V;
      const unsigned rj = r / q2;
      int fa, fc;                                                             // out[i][j] = flipped[fa][fc]
      rot90_source(s.k, (int)(rj / R1), (int)(rj % R1), R0, R1, fa, fc);
      if (s.flip & 1) fa = R0 - 1 - fa;
      if (s.flip & 2) fc = R1 - 1 - fc;
      float v[V];
      unsigned lv[V];
      volume_feed_gather<V>(s, c0, c1, c2, fa, fc, l, R2, v, lv);
      feed_store<V>(img + (long)r * V, lab + (long)r * V, v, lv);
    }
    return;
  }
  const AffineFrame frame = affine_frame(R0, R1, R2, c0 - s.l0, c1 - s.l1, c2 - s.l2);
  const AffineVolume vol = {rec.n0, s.n1, s.n2, 0, (long)s.n1 * s.n2, s.n2};
  for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < voxels; e += gridDim.x * blockDim.x) {
    int i, j, l;
    affine_thread_voxel(e, R1, R2, i, j, l);
    int fa, fc;                                                               // out[i][j] = flipped[fa][fc]
    rot90_source(s.k, i, j, R0, R1, fa, fc);
    if (s.flip & 1) fa = R0 - 1 - fa;
    if (s.flip & 2) fc = R1 - 1 - fc;
    const AffineTaps taps = affine_taps(fa, fc, (s.flip & 4) ? R2 - 1 - l : l, rec.m, frame, vol);
    const unsigned r = ((unsigned)i * R1 + j) * R2 + l;                       // the output voxel
    const float m = affine_value(s.image, taps) * s.mul;                      // two roundings
    img[r] = m + s.add;
    lab[r] = (long long)(s.label[taps.label] * taps.labelled);
  }
}

// ---- the BraTS chain (crop_rotflip_channels_kernel: rot90 -> flip -> zero padding -> crop, images [C][n0][n1][n2] with ONE label) with the
// stage about the patch centre (DESIGN.md §2 "Affine stage of the BraTS feed").  The sampled volume is Y = flip(rot90(x, k), axis) of
// extents (r0, r1, n2); it is never materialised: crop_feed_row gives its origin and its signed strides in the source.  A tap outside Y
// counts as 0, which is the zero padding as well.  A sample either has the stage (`affine` = 1) or it does not: without it the sample
// goes through crop_feed_gather, as in crop_rotflip_channels_kernel, and its values are copied.  No mul / add.
struct CropAffineSample {
  FeedSample f;              // as for crop_rotflip_channels_kernel
  int affine;                // 1: the sample has the affine stage; 0: m is not read
  double m[9];               // M, row-major
};

struct CropAffineBatch {
  CropAffineSample s[kFeedMaxBatch];     // 144 B a record: 2,304 B of the 4 KB kernel-argument block
};

// image_out [B][C][R0][R1][R2] fp32, label_out [B][R0][R1][R2] int64.  grid (x, B): one sample per blockIdx.y, so its record and `affine`
// are wave-uniform.  V (4: R2 % 4 == 0 and both outputs 16-byte aligned) is the form of the INTEGER path, one thread per V consecutive
// depth voxels as in crop_rotflip_channels_kernel<V>.  An affine sample takes one thread per output voxel in both instances
// (affine_thread_voxel): the taps come from the definition once, the channel loop is affine_value with channel stride n0 n1 n2.
// No LDS, no atomics.
template <int V>
__global__ __launch_bounds__(256) void crop_rotflip_affine_kernel(CropAffineBatch fb, float* __restrict__ image_out, long long* __restrict__ label_out,
                                                                  int C, int R0, int R1, int R2) {
  static_assert(V == 1 || V == 4, "one voxel or one quad per thread");
  const int b = blockIdx.y;
  const CropAffineSample& rec = fb.s[b];
  const FeedSample& s = rec.f;
  const unsigned voxels = (unsigned)R0 * R1 * R2;                             // channel stride of the output; the launcher keeps it below 2^31
  // extents after rot90: odd k swaps axes 0 and 1
  const int r0 = (s.k & 1) ? s.n1 : s.n0, r1 = (s.k & 1) ? s.n0 : s.n1;
  float* __restrict__ img = image_out + (long)b * C * voxels;
  long long* __restrict__ lab = label_out + (long)b * voxels;
  if (!rec.affine) {
    const int q2 = R2 / V;
    for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < voxels / V; r += gridDim.x * blockDim.x) {
      const int l = (int)(r % q2) * V;
      const unsigned rj = r / q2;
      const long e = (long)r * V;                                             // = (i * R1 + j) * R2 + l
      crop_feed_gather<V>(s, r0, r1, C, (int)(rj / R1), (int)(rj % R1), l, img + e, voxels, lab + e);
    }
    return;
  }
  const long cs = (long)s.n0 * s.n1 * s.n2;                                   // channel stride of the source
  // Y[a][c][d] = source[origin + a * stride0 + c * stride1 + d]: the map is affine in (a, c), so three evaluations give it (they index nothing)
  const long origin = crop_feed_row(s, r0, r1, 0, 0);
  const AffineVolume vol = {r0, r1, s.n2, origin, crop_feed_row(s, r0, r1, 1, 0) - origin, crop_feed_row(s, r0, r1, 0, 1) - origin};
  const AffineFrame frame = affine_frame(R0, R1, R2, s.c0 - s.p0, s.c1 - s.p1, s.c2 - s.p2);
  for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < voxels; e += gridDim.x * blockDim.x) {
    int i, j, l;
    affine_thread_voxel(e, R1, R2, i, j, l);
    const AffineTaps taps = affine_taps(i, j, l, rec.m, frame, vol);
    const unsigned r = ((unsigned)i * R1 + j) * R2 + l;                       // the output voxel
    const unsigned lraw = s.label[taps.label];
    const float* __restrict__ p = s.image;                                    // channel ch of the source ...
    float* __restrict__ o = img + r;                                          // ... and of the output voxel
    for (int ch = 0; ch < C; ++ch, p += cs, o += voxels) *o = affine_value(p, taps);
    lab[r] = (long long)(lraw * taps.labelled);
  }
}

}  // namespace icl
