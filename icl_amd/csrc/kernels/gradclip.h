// gradclip.h — gradient clipping by the global 2-norm (torch.nn.utils.clip_grad_norm_ semantics), measured from dense gradients AND from
// gradients that are still factored (G = g^T x, g [M][N], x [M][K]: ops.FactoredGrads) without multiplying them out:
//   |g^T x|_F^2 = sum_{r,s} (g_r . g_s)(x_r . x_s)            two M x M Gram matrices over vectors of length N and K
// Every square, product and sum is formed in DOUBLE: the off-diagonal terms have either sign and cancel (two rows g_1 = -g_0,
// x_1 = (1 + 2^-5) x_0: condition number ~4e3; an fp32 Gram is hundreds of fp32 ulps off there).  No float atomics: every workgroup writes
// its partial to a workspace slot fixed by its index and the sums run in a fixed order, so two runs give the same bits.
//   gradclip_sumsq_multi_kernel   dense sum of squares, up to 48 tensors per launch, one double per (tensor, chunk)
//   gradclip_gram_kernel          partial Gram entries (r <= s) of g and of x per slab of the long axis
//   gradclip_gram_combine_kernel  slab partials summed in slab order, then sum_{r<=s} w_rs GG_rs XX_rs (w = 1 on the diagonal, 2 off it)
//   gradclip_finish_kernel        one workgroup: the sum of all partials, total_norm = (float)sqrt(sum), coef = min(1, max_norm / (norm + 1e-6))
//   gradclip_scale_multi_kernel   dst = src * coef (coef read from device memory), in place or out of place, up to 48 tensors per launch
// The dense kernels are HBM streams (4 B per element); the fp64 arithmetic hides behind the loads.
#pragma once

namespace icl {

constexpr int kGcMulti = 48;

// the sum of the 256 threads' values, in a fixed tree order; `sm` holds 256 doubles.  Every thread of the workgroup calls it.
__device__ __forceinline__ double gc_block_sum(double v, double* sm) {
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  return sm[0];
}

__device__ __forceinline__ double gc_sq(float v) {
  const double d = (double)v;
  return d * d;
}

// float4 body when the pointer is 16-byte aligned, scalar tail, scalar path for misaligned views (the structure of adamw_range)
__device__ __forceinline__ double gc_sumsq_range(const float* __restrict__ g, long n, long start, long stride) {
  double acc = 0.0;
  long tail = start;
  if ((((unsigned long long)g) & 15ull) == 0) {
    const long n4 = n >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (long i = start; i < n4; i += stride) {
      const float4 v = g4[i];
      acc += gc_sq(v.x);
      acc += gc_sq(v.y);
      acc += gc_sq(v.z);
      acc += gc_sq(v.w);
    }
    tail = (n4 << 2) + start;
  }
  for (long i = tail; i < n; i += stride) acc += gc_sq(g[i]);
  return acc;
}

struct GcSumsqMulti {
  const float* g[kGcMulti];
  long n[kGcMulti];
};

// grid (chunks, tensors), block 256: partial[tensor * chunks + chunk] = this workgroup's share of sum g^2 (0 when it has none)
__global__ __launch_bounds__(256) void gradclip_sumsq_multi_kernel(GcSumsqMulti t, double* __restrict__ partial) {
  __shared__ double sm[256];
  const int k = blockIdx.y;
  const double acc = gc_sumsq_range(t.g[k], t.n[k], (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
  const double tot = gc_block_sum(acc, sm);
  if (threadIdx.x == 0) partial[(long)k * gridDim.x + blockIdx.x] = tot;
}

// ---- partial Gram matrices of a [M][L] (row-major; side 0: g with L = N, side 1: x with L = K).  grid (slabs, chunk pairs, 2), block 256.
// A workgroup takes one slab of `slab` columns and one pair (ca <= cb) of chunks of 32 rows; the rows are staged through LDS in pieces
// of 128 columns, transposed ([column][row], stride 33: the staging stores and the reads of 32 consecutive rows are conflict-free on the
// 64 banks); thread t owns the 2 x 2 entries rows 2 (t / 16) .., columns 2 (t % 16) .. of the 32 x 32 block and keeps them in double.
// Entries r <= s go to ws[side][slab][r * M + s]; the others are never written nor read.
constexpr int kGcRows = 32, kGcCols = 128, kGcStride = kGcRows + 1;

__device__ __forceinline__ void gc_stage(float (*dst)[kGcStride], const float* __restrict__ a, int M, int L, int r0, int c0, int c_end) {
  for (int it = threadIdx.x; it < kGcRows * kGcCols; it += 256) {
    const int row = it / kGcCols, c = it % kGcCols;
    dst[c][row] = (r0 + row < M && c0 + c < c_end) ? a[(long)(r0 + row) * L + c0 + c] : 0.f;
  }
}

__global__ __launch_bounds__(256) void gradclip_gram_kernel(const float* __restrict__ g, const float* __restrict__ x, int M, int N, int K,
                                                            int slab_g, int slab_x, int nslab_g, int nslab_x, double* __restrict__ ws) {
  __shared__ float as[kGcCols][kGcStride];
  __shared__ float bs[kGcCols][kGcStride];
  const int side = blockIdx.z;
  const float* __restrict__ a = side ? x : g;
  const int L = side ? K : N, slab = side ? slab_x : slab_g, nslab = side ? nslab_x : nslab_g;
  if ((int)blockIdx.x >= nslab) return;      // uniform: the two sides share one grid
  const int nch = (M + kGcRows - 1) / kGcRows;
  int ca = 0, rem = blockIdx.y;
  while (rem >= nch - ca) {
    rem -= nch - ca;
    ++ca;
  }
  const int cb = ca + rem;
  const int r0 = ca * kGcRows, s0 = cb * kGcRows;
  const int ri = (threadIdx.x >> 4) * 2, si = (threadIdx.x & 15) * 2;
  const int c_begin = blockIdx.x * slab;
  const int c_end = (c_begin + slab < L) ? c_begin + slab : L;
  const bool live = s0 + si < M && r0 + ri <= s0 + si;      // (both even: a 2 x 2 block has an entry r <= s exactly when its first has)
  float (*bp)[kGcStride] = (ca == cb) ? as : bs;
  double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
  for (int c0 = c_begin; c0 < c_end; c0 += kGcCols) {
    __syncthreads();
    gc_stage(as, a, M, L, r0, c0, c_end);
    if (ca != cb) gc_stage(bs, a, M, L, s0, c0, c_end);
    __syncthreads();
    if (!live) continue;
    const int cc = (c_end - c0 < kGcCols) ? c_end - c0 : kGcCols;
    for (int c = 0; c < cc; ++c) {
      const double u0 = (double)as[c][ri], u1 = (double)as[c][ri + 1];
      const double v0 = (double)bp[c][si], v1 = (double)bp[c][si + 1];
      a00 += u0 * v0;
      a01 += u0 * v1;
      a10 += u1 * v0;
      a11 += u1 * v1;
    }
  }
  if (!live) return;
  double* __restrict__ out = ws + ((side ? (long)nslab_g : 0l) + blockIdx.x) * ((long)M * M);
  const int r = r0 + ri, s = s0 + si;
  out[(long)r * M + s] = a00;                            // r <= s < M for every live thread
  if (s + 1 < M) out[(long)r * M + s + 1] = a01;
  if (r < s) out[(long)(r + 1) * M + s] = a10;           // (r + 1 <= s < M)
  if (s + 1 < M) out[(long)(r + 1) * M + s + 1] = a11;   // (r + 1 <= s + 1 < M)
}

// the sum of p[0], p[stride], ..., p[(n - 1) stride] in that order; eight loads are in flight before their adds (one thread walks the
// slabs of its entry: issued one by one the loads' latencies would add up)
__device__ __forceinline__ double gc_slab_sum(const double* __restrict__ p, long stride, int n) {
  double acc = 0.0;
  int sl = 0;
  for (; sl + 8 <= n; sl += 8) {
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[(long)(sl + j) * stride];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += v[j];
  }
  for (; sl < n; ++sl) acc += p[(long)sl * stride];
  return acc;
}

// grid ceil(M^2 / 256), block 256: thread e = r M + s (r <= s) sums its entry's slab partials in slab order and forms w GG XX; the
// workgroup's sum goes to partial[blockIdx.x]
__global__ __launch_bounds__(256) void gradclip_gram_combine_kernel(const double* __restrict__ ws, int M, int nslab_g, int nslab_x,
                                                                    double* __restrict__ partial) {
  __shared__ double sm[256];
  const long mm = (long)M * M;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  double term = 0.0;
  if (e < mm) {
    const int r = (int)(e / M), s = (int)(e % M);
    if (r <= s) {
      const double gg = gc_slab_sum(ws + e, mm, nslab_g);
      const double xx = gc_slab_sum(ws + (long)nslab_g * mm + e, mm, nslab_x);
      term = (r == s ? 1.0 : 2.0) * (gg * xx);
    }
  }
  const double tot = gc_block_sum(term, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// one workgroup of 256: thread t sums partial[t], partial[t + 256], ... in that order, then the tree.  clip = {total_norm, coef}: the
// norm rounded once from double; the coefficient in fp32 as torch evaluates it (max_norm / (total_norm + 1e-6), clamped to at most 1; a
// NaN stays a NaN, an infinite norm gives 0)
__global__ __launch_bounds__(256) void gradclip_finish_kernel(const double* __restrict__ partial, long count, float max_norm,
                                                              float* __restrict__ clip) {
  __shared__ double sm[256];
  double acc = 0.0;
  for (long i = threadIdx.x; i < count; i += 256) acc += partial[i];
  const double tot = gc_block_sum(acc, sm);
  if (threadIdx.x == 0) {
    const float total_norm = (float)sqrt(tot);
    const float c = max_norm / (total_norm + 1e-6f);
    clip[0] = total_norm;
    clip[1] = c > 1.0f ? 1.0f : c;
  }
}

struct GcScaleMulti {
  float* dst[kGcMulti];
  const float* src[kGcMulti];
  long n[kGcMulti];
};

// grid (chunks, tensors), block 256: dst = src * clip[1].  An unclipped step (coef == 1) in place returns at once: launches, no traffic.
__global__ __launch_bounds__(256) void gradclip_scale_multi_kernel(GcScaleMulti t, const float* __restrict__ clip) {
  const int k = blockIdx.y;
  const float coef = clip[1];
  float* dst = t.dst[k];
  const float* src = t.src[k];
  if (coef == 1.0f && dst == src) return;
  const long n = t.n[k], start = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  long tail = start;
  if (((((unsigned long long)dst) | ((unsigned long long)src)) & 15ull) == 0) {
    const long n4 = n >> 2;
    float4* d4 = reinterpret_cast<float4*>(dst);
    const float4* s4 = reinterpret_cast<const float4*>(src);
    for (long i = start; i < n4; i += stride) {
      float4 v = s4[i];
      v.x *= coef;
      v.y *= coef;
      v.z *= coef;
      v.w *= coef;
      d4[i] = v;
    }
    tail = (n4 << 2) + start;
  }
  for (long i = tail; i < n; i += stride) dst[i] = src[i] * coef;
}

}  // namespace icl
