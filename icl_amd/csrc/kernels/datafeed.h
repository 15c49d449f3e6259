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
    int a = s.c0 + i - s.p0, c = s.c1 + j - s.p1;
    const int d = s.c2 + l - s.p2;
    float v = 0.f;
    long long lab = 0;
    if (a >= 0 && a < r0 && c >= 0 && c < r1 && d >= 0 && d < s.n2) {
      if (s.flip_axis == 0) a = r0 - 1 - a;
      else if (s.flip_axis == 1) c = r1 - 1 - c;
      // rot90 on axes (0, 1): rotated[a][c] = source[sa][sc]
      int sa, sc;
      switch (s.k & 3) {
        case 0: sa = a; sc = c; break;
        case 1: sa = c; sc = s.n1 - 1 - a; break;
        case 2: sa = s.n0 - 1 - a; sc = s.n1 - 1 - c; break;
        default: sa = s.n0 - 1 - c; sc = a; break;
      }
      const long src = ((long)sa * s.n1 + sc) * s.n2 + d;
      v = s.image[src];
      lab = (long long)s.label[src];
    }
    image_out[e] = v;
    label_out[e] = lab;
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
        switch (s.k & 3) {          // rot90: rotated[a][c] = source[sa][sc] (the maps of crop_rotflip_kernel)
          case 0: sa = a; sc = c; break;
          case 1: sa = c; sc = s.n1 - 1 - a; break;
          case 2: sa = s.n0 - 1 - a; sc = s.n1 - 1 - c; break;
          default: sa = s.n0 - 1 - c; sc = a; break;
        }
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

}  // namespace icl
