// loss_point.h — the voxel-wise losses of utils/losses.py: softmax KL divergence (softmax_kl_loss :93-112, compute_kl_loss :334-346), entropy
// (entropy_loss :33-39, entropy_loss_map :62-65, entropy_minmization :321-325, entropy_map :328-331) and the focal loss (FocalLoss :149-183),
// forward and backward.
//
// Unlike Dice (loss.h) no coefficient of these gradients depends on a global sum: the forward pass reduces ONE scalar per call (and may
// write a per-voxel map), the backward pass needs only the upstream gradient — nothing is kept between the two.  The reference materialises
// the soft-max, its log and the one-hot or second soft-max as full [B, nc, S] tensors and runs a chain of element-wise launches in both
// passes; here each pass reads the logits once (class walks after the first hit the cache) and writes only its result.
//
// Tensors are (outer, nc, inner): the class axis has stride `inner`, voxel e = o * inner + i sits at o * nc * inner + i.  inner = S is
// dim 1 of [B, nc, ...]; inner = 1 is the last axis of [M, nc] (correct, strided loads — its speed is no goal).
// As loss.h: 256 threads, grid-stride over the voxels, one partial per block, a one-block finalize that adds the partials in a fixed
// order (here in double); no atomics, nothing pre-zeroed, bit-reproducible.  NCMAX = 4 | 16: the classes of a voxel in registers; NCMAX = 0: the
// class-walking body (17 .. 256 classes, online soft-max normaliser), which holds nothing that grows with nc.
#pragma once

namespace icl {

constexpr float kEntropyEps = 1e-6f;     // log(p + 1e-6) of the reference's entropy functions

// The nc values of one voxel: a register copy (NCMAX > 0) or the strided address itself (NCMAX = 0).
template <int NCMAX>
struct PointRow {
  float v[NCMAX];
  __device__ __forceinline__ void load(const float* __restrict__ p, int nc, long stride) {
#pragma unroll
    for (int c = 0; c < NCMAX; ++c) v[c] = c < nc ? p[(long)c * stride] : 0.f;
  }
  __device__ __forceinline__ float at(int c) const { return v[c]; }
  // max and sum of exp(v - max)
  __device__ __forceinline__ void norm(int nc, float& m, float& sum) const {
    m = v[0];
#pragma unroll
    for (int c = 1; c < NCMAX; ++c)
      if (c < nc) m = fmaxf(m, v[c]);
    sum = 0.f;
#pragma unroll
    for (int c = 0; c < NCMAX; ++c)
      if (c < nc) sum += expf(v[c] - m);
  }
};
template <>
struct PointRow<0> {
  const float* p;
  long stride;
  __device__ __forceinline__ void load(const float* __restrict__ q, int, long s) { p = q; stride = s; }
  __device__ __forceinline__ float at(int c) const { return p[(long)c * stride]; }
  __device__ __forceinline__ void norm(int nc, float& m, float& sum) const { softmax_norm_strided(p, nc, stride, m, sum); }
};

// the class loop of a body: fully unrolled over NCMAX with the tail masked, or a plain walk over nc (NCMAX = 0)
#define ICL_POINT_CLASSES(c) _Pragma("unroll NCMAX ? NCMAX : 1") for (int c = 0; c < (NCMAX ? NCMAX : nc); ++c) if (c < nc)

// The block's sum in a fixed tree order, in double: a thread's fp32 accumulator holds only a handful of voxels, everything above it is
// added in double, so that the value is rounded to fp32 once, at the end (a mean over 10^6 voxels summed in fp32 lands an ulp off).
// Every thread of the block calls it.
__device__ __forceinline__ double point_block_sum(double v) {
  __shared__ double sm[256];
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  return sm[0];
}
__device__ __forceinline__ void point_block_partial(float v, float* __restrict__ dst) {
  const double t = point_block_sum((double)v);
  if (threadIdx.x == 0) *dst = (float)t;
}

// out[0] = scale * (sum of the nblk partials): thread t adds partials t, t + 256, ... in order, then the block sum above; one rounding
__global__ __launch_bounds__(256) void point_finalize_kernel(const float* __restrict__ part, int nblk, float* __restrict__ out, double scale) {
  double v = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) v += (double)part[b];
  const double t = point_block_sum(v);
  if (threadIdx.x == 0) out[0] = (float)(t * scale);
}

// ---------------------------------------------------------------- KL:  w_fwd * KL(q || p) + w_rev * KL(p || q),  p = softmax(a), q = softmax(b)
// The logs are v - lse, never log(softmax): a class whose probability underflows contributes 0 * finite = 0 (torch's xlogy convention).
// The soft-max normalisers of a voxel's two rows and its two divergences, kf = KL_v(q || p) and kr = KL_v(p || q): one evaluation for the
// forward and the backward pass.
template <int NCMAX>
struct PointKL {
  float ma, mb, lsa, lsb, ia, ib, kf, kr;
  __device__ __forceinline__ void eval(const PointRow<NCMAX>& ra, const PointRow<NCMAX>& rb, int nc) {
    float sa, sb;
    ra.norm(nc, ma, sa);
    rb.norm(nc, mb, sb);
    lsa = ma + logf(sa);
    lsb = mb + logf(sb);
    ia = 1.0f / sa;
    ib = 1.0f / sb;
    kf = 0.f;
    kr = 0.f;
    ICL_POINT_CLASSES(c) {
      const float x = ra.at(c), y = rb.at(c);
      const float d = (y - lsb) - (x - lsa);            // log q - log p
      kf += expf(y - mb) * ib * d;
      kr -= expf(x - ma) * ia * d;
    }
  }
};

template <int NCMAX>
__global__ __launch_bounds__(256) void point_kl_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ part,
                                                           long outer, int nc, long inner, float w_fwd, float w_rev) {
  const long total = outer * inner;
  float acc = 0.f;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long o = e / inner, base = o * nc * inner + (e - o * inner);
    PointRow<NCMAX> ra, rb;
    ra.load(a + base, nc, inner);
    rb.load(b + base, nc, inner);
    PointKL<NCMAX> k;
    k.eval(ra, rb, nc);
    acc += w_fwd * k.kf + w_rev * k.kr;
  }
  point_block_partial(acc, part + blockIdx.x);
}

// ga = g/N [ w_fwd (p - q) + w_rev p ((log p - log q) - KL_v(p||q)) ],  gb the same with the roles and weights swapped; either may be NULL
template <int NCMAX>
__global__ __launch_bounds__(256) void point_kl_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ gout,
                                                           float* __restrict__ ga, float* __restrict__ gb, long outer, int nc, long inner,
                                                           float w_fwd, float w_rev, float inv_elems) {
  const long total = outer * inner;
  const float g = gout[0] * inv_elems;
  const float gf = g * w_fwd, gr = g * w_rev;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long o = e / inner, base = o * nc * inner + (e - o * inner);
    PointRow<NCMAX> ra, rb;
    ra.load(a + base, nc, inner);
    rb.load(b + base, nc, inner);
    PointKL<NCMAX> k;
    k.eval(ra, rb, nc);
    ICL_POINT_CLASSES(c) {
      const float x = ra.at(c), y = rb.at(c);
      float d = (y - k.lsb) - (x - k.lsa);
      const float p = expf(x - k.ma) * k.ia, q = expf(y - k.mb) * k.ib;
      // one difference each, pinned (ICL_PIN1: an empty asm, no instruction), used with both signs: left alone hipcc forms (d, -d) as a
      // packed add with crossed halves, the form no kernel of the library keeps (tests/test_host_logic.py)
      float pq = p - q;
      ICL_PIN1(d);
      ICL_PIN1(pq);
      if (ga) ga[base + (long)c * inner] = gf * pq - gr * p * (d + k.kr);
      if (gb) gb[base + (long)c * inner] = gf * q * (d - k.kf) - gr * pq;
    }
  }
}

// ---------------------------------------------------------------- entropy:  H_v = -sum_c p_c log(p_c + 1e-6),  p = x or softmax(x)
// out (mean over the voxels, through `part` + point_finalize_kernel) and / or map[e] = scale * H_v; either may be NULL.
template <int NCMAX>
__global__ __launch_bounds__(256) void point_entropy_fwd_kernel(const float* __restrict__ x, float* __restrict__ part, float* __restrict__ map,
                                                                long outer, int nc, long inner, int from_logits, float scale) {
  const long total = outer * inner;
  float acc = 0.f;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long o = e / inner, base = o * nc * inner + (e - o * inner);
    PointRow<NCMAX> r;
    r.load(x + base, nc, inner);
    float m = 0.f, inv = 1.f;
    if (from_logits) {
      float s;
      r.norm(nc, m, s);
      inv = 1.0f / s;
    }
    float h = 0.f;
    ICL_POINT_CLASSES(c) {
      const float v = r.at(c);
      const float p = from_logits ? expf(v - m) * inv : v;
      h -= p * logf(p + kEntropyEps);
    }
    if (map) map[e] = scale * h;
    acc += h;
  }
  if (part) point_block_partial(acc, part + blockIdx.x);
}

// d/dp_c = -coef_v [log(p_c + 1e-6) + p_c / (p_c + 1e-6)] (finite at p = 0), coef_v = scale (gout / V + gmap[e]); with from_logits chained
// through the soft-max: p_c (d_c - sum d p).  gout / gmap: the upstream gradient of the mean / of the map, either may be NULL.
template <int NCMAX>
__global__ __launch_bounds__(256) void point_entropy_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gout,
                                                                const float* __restrict__ gmap, float* __restrict__ gx, long outer, int nc,
                                                                long inner, int from_logits, float scale, float inv_vox) {
  const long total = outer * inner;
  const float gmean = gout ? gout[0] * inv_vox : 0.f;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long o = e / inner, base = o * nc * inner + (e - o * inner);
    PointRow<NCMAX> r;
    r.load(x + base, nc, inner);
    const float coef = scale * (gmean + (gmap ? gmap[e] : 0.f));
    float m = 0.f, inv = 1.f, dot = 0.f;
    if (from_logits) {
      float s;
      r.norm(nc, m, s);
      inv = 1.0f / s;
      ICL_POINT_CLASSES(c) {
        const float p = expf(r.at(c) - m) * inv;
        dot -= coef * (logf(p + kEntropyEps) + p / (p + kEntropyEps)) * p;
      }
    }
    ICL_POINT_CLASSES(c) {
      const float v = r.at(c);
      const float p = from_logits ? expf(v - m) * inv : v;
      const float d = -coef * (logf(p + kEntropyEps) + p / (p + kEntropyEps));
      gx[base + (long)c * inner] = from_logits ? p * (d - dot) : d;
    }
  }
}

// ---------------------------------------------------------------- focal:  loss_v = -alpha_y (1 - pt)^gamma log pt,  pt = softmax(a)_y
// A label outside [0, nc) indexes nothing: that voxel adds 0 to the value and gets a zero gradient (it still counts in the mean).
// gamma == 0: factor 1 even at pt = 1; gamma == 2: a square, not a power function.
__device__ __forceinline__ float focal_factor(float pt, float gamma) {
  const float u = 1.0f - pt;
  if (gamma == 0.f) return 1.0f;
  if (gamma == 2.f) return u * u;
  // u^gamma as exp(gamma log u), relative error |gamma log u| * 2^-24 (1e-6 at u = 1e-5, where the factor itself is 3e-8 for gamma = 1.5);
  // the library's powf carries packed adds with crossed halves, the form no kernel here keeps (tests/test_host_logic.py)
  return u > 0.f ? expf(gamma * logf(u)) : 0.f;
}

template <int NCMAX>
__global__ __launch_bounds__(256) void point_focal_fwd_kernel(const float* __restrict__ a, const long long* __restrict__ labels,
                                                              const float* __restrict__ alpha, float* __restrict__ part, long outer, int nc,
                                                              long inner, float gamma) {
  const long total = outer * inner;
  float acc = 0.f;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long long y = labels[e];
    if (y < 0 || y >= nc) continue;
    const long o = e / inner, base = o * nc * inner + (e - o * inner);
    PointRow<NCMAX> r;
    r.load(a + base, nc, inner);
    float m, s;
    r.norm(nc, m, s);
    float ay = 0.f;
    if constexpr (NCMAX != 0) {
      ICL_POINT_CLASSES(c)
        if (c == (int)y) ay = r.at(c);
    } else {
      ay = r.at((int)y);
    }
    const float logpt = (ay - m) - logf(s);          // <= 0: s >= 1 and ay <= m
    const float pt = expf(logpt);
    acc -= (alpha ? alpha[y] : 1.0f) * focal_factor(pt, gamma) * logpt;
  }
  point_block_partial(acc, part + blockIdx.x);
}

// The reference takes pt from .data: (1 - pt)^gamma is a CONSTANT of the backward pass.  ga_c = g alpha_y (1 - pt)^gamma (p_c - [c == y]) * inv
// (inv = 1 / V for the mean, 1 for the sum).
template <int NCMAX>
__global__ __launch_bounds__(256) void point_focal_bwd_kernel(const float* __restrict__ a, const long long* __restrict__ labels,
                                                              const float* __restrict__ alpha, const float* __restrict__ gout,
                                                              float* __restrict__ ga, long outer, int nc, long inner, float gamma, float inv) {
  const long total = outer * inner;
  const float g = gout[0] * inv;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long o = e / inner, base = o * nc * inner + (e - o * inner);
    const long long y = labels[e];
    if (y < 0 || y >= nc) {
      for (int c = 0; c < nc; ++c) ga[base + (long)c * inner] = 0.f;
      continue;
    }
    PointRow<NCMAX> r;
    r.load(a + base, nc, inner);
    float m, s;
    r.norm(nc, m, s);
    const float is = 1.0f / s;
    float ay = 0.f;
    if constexpr (NCMAX != 0) {
      ICL_POINT_CLASSES(c)
        if (c == (int)y) ay = r.at(c);
    } else {
      ay = r.at((int)y);
    }
    const float pt = expf((ay - m) - logf(s));
    const float k = g * (alpha ? alpha[y] : 1.0f) * focal_factor(pt, gamma);
    ICL_POINT_CLASSES(c) {
      const float p = expf(r.at(c) - m) * is;
      ga[base + (long)c * inner] = k * (p - (c == (int)y ? 1.f : 0.f));
    }
  }
}

#undef ICL_POINT_CLASSES

}  // namespace icl
