// adamw.h — fused AdamW (torch.optim.AdamW semantics, amsgrad = False, maximize = False), per fp32 element:
//   p1 = p * decay;   m' = m + (g - m) * omb1;   v' = v * beta2 + omb2 * g * g;
//   denom = sqrt(v') / bc2_sqrt + eps;   p' = p1 - step_size * (m' / denom)
// The host forms decay = 1 - lr wd, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), omb1 = 1 - beta1, omb2 = 1 - beta2 in
// double and rounds each once to fp32 — where torch rounds them (1.0f - 0.999f on the device is 5e-5 off float(1 - 0.999)).  IEEE sqrtf
// and division: the kernels are HBM streams (28 B per parameter dense, 24 B factored), the arithmetic is free.
// first != 0: m and v count as 0 and are NEVER read (the state tensors may be uninitialised).
// hyper_dev (optional): {decay, step_size, bc2_sqrt} read from device memory, so a captured hipGraph follows the host's schedule and
// the bias corrections of the step count — what lr_dev is for the SGD kernels (optim.h).
#pragma once

namespace icl {

struct AdamwHyper {
  float decay, step_size, bc2_sqrt, beta2, omb1, omb2, eps;
};

__device__ __forceinline__ AdamwHyper adamw_hyper(AdamwHyper h, const float* __restrict__ hyper_dev) {
  if (hyper_dev) {
    h.decay = hyper_dev[0];
    h.step_size = hyper_dev[1];
    h.bc2_sqrt = hyper_dev[2];
  }
  return h;
}

__device__ __forceinline__ void adamw_update1(float& p, float g, float& m, float& v, const AdamwHyper& h) {
  const float p1 = p * h.decay;
  m = m + (g - m) * h.omb1;
  v = v * h.beta2 + h.omb2 * g * g;
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p = p1 - h.step_size * (m / denom);
}

__device__ __forceinline__ void adamw_update4(float4& p, const float4& g, float4& m, float4& v, const AdamwHyper& h) {
  adamw_update1(p.x, g.x, m.x, v.x, h);
  adamw_update1(p.y, g.y, m.y, v.y, h);
  adamw_update1(p.z, g.z, m.z, v.z, h);
  adamw_update1(p.w, g.w, m.w, v.w, h);
}

// the structure of sgd_range (optim.h): float4 body when all four pointers are 16-byte aligned, scalar tail, scalar path otherwise
__device__ __forceinline__ void adamw_range(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                            long n, long start, long stride, const AdamwHyper& h, int first) {
  const bool al = ((((unsigned long long)p) | ((unsigned long long)g) | ((unsigned long long)m) | ((unsigned long long)v)) & 15ull) == 0;
  long tail = start;      // first element of the scalar loop
  if (al) {
    const long n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long i = start; i < n4; i += stride) {
      float4 pv = p4[i], mv = first ? zero : m4[i], vv = first ? zero : v4[i];
      adamw_update4(pv, g4[i], mv, vv, h);
      p4[i] = pv;
      m4[i] = mv;
      v4[i] = vv;
    }
    tail = (n4 << 2) + start;
  }
  for (long i = tail; i < n; i += stride) {
    float pv = p[i], mv = first ? 0.f : m[i], vv = first ? 0.f : v[i];
    adamw_update1(pv, g[i], mv, vv, h);
    p[i] = pv;
    m[i] = mv;
    v[i] = vv;
  }
}

// dense: reads p, g, m, v and writes p, m, v (28 B per parameter), grid-stride
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, AdamwHyper h, int first,
                                                    const float* __restrict__ hyper_dev) {
  h = adamw_hyper(h, hyper_dev);
  adamw_range(p, g, m, v, n, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x, h, first);
}

constexpr int kAdamwMulti = 48;
struct AdamwMulti {
  float* p[kAdamwMulti];
  const float* g[kAdamwMulti];
  float* m[kAdamwMulti];
  float* v[kAdamwMulti];
  long n[kAdamwMulti];
};

// grid (chunks, tensors): every small tensor gets gridDim.x workgroups (as sgd_momentum_multi_kernel)
__global__ __launch_bounds__(256) void adamw_multi_kernel(AdamwMulti t, AdamwHyper h, int first, const float* __restrict__ hyper_dev) {
  h = adamw_hyper(h, hyper_dev);
  const int k = blockIdx.y;
  adamw_range(t.p[k], t.g[k], t.m[k], t.v[k], t.n[k], (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x, h, first);
}

// ---- AdamW step of a Linear weight p [N][K] whose gradient is still FACTORED: gg[n][k] = sum_r g[r][n] * x[r][k], summed in fp32 in row
// order r = 0 .. M-1.  Staging and thread map of sgd_factored_small_kernel (optim.h): 16 x 256 tiles, the factor slices in LDS in
// chunks of 32 rows, any M >= 1, K % 4 == 0; grid (ceil(K/256), ceil(N/16)), block 256: thread = float4 column kq (0..63) x row lane rl
// (rows 4*rl .. 4*rl+3).  The p / m / v loads are issued before the products (their HBM latency overlaps the staging and the FMAs), with
// non-temporal loads and stores (each is touched once per step): 24 B per weight, the 764 MB gradient of a 13,824^2 matrix is never formed.
constexpr int kAvRows = 16, kAvCols = 256, kAvChunk = 32;

__global__ __launch_bounds__(256) void adamw_factored_kernel(float* __restrict__ p, float* __restrict__ mom, float* __restrict__ var,
                                                             const float* __restrict__ g, const float* __restrict__ x, int M, int N, int K,
                                                             AdamwHyper h, int first, const float* __restrict__ hyper_dev) {
  __shared__ float4 xs[kAvChunk][kAvCols / 4];
  __shared__ float gs[kAvChunk][kAvRows];
  h = adamw_hyper(h, hyper_dev);
  const int n0 = blockIdx.y * kAvRows, k0 = blockIdx.x * kAvCols;
  const int kq = threadIdx.x & 63, rl = threadIdx.x >> 6;
  float4 acc[4], pv[4], mv[4], vv[4];
  const bool col_ok = k0 + kq * 4 < K;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = n0 + rl * 4 + r;
    acc[r] = pv[r] = mv[r] = vv[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (col_ok && n < N) {
      const long idx = (long)n * K + k0 + kq * 4;
      pv[r] = icl_nt_load4(p + idx);
      if (!first) {
        mv[r] = icl_nt_load4(mom + idx);
        vv[r] = icl_nt_load4(var + idx);
      }
    }
  }
  for (int m0 = 0; m0 < M; m0 += kAvChunk) {
    __syncthreads();
    for (int it = threadIdx.x; it < kAvChunk * (kAvCols / 4); it += 256) {
      const int m = it / (kAvCols / 4), q = it % (kAvCols / 4);
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m0 + m < M && k0 + q * 4 < K) t = *reinterpret_cast<const float4*>(x + (long)(m0 + m) * K + k0 + q * 4);
      xs[m][q] = t;
    }
    for (int it = threadIdx.x; it < kAvChunk * kAvRows; it += 256) {
      const int m = it / kAvRows, r = it % kAvRows;
      gs[m][r] = (m0 + m < M && n0 + r < N) ? g[(long)(m0 + m) * N + n0 + r] : 0.f;
    }
    __syncthreads();
    const int mc = (M - m0 < kAvChunk) ? M - m0 : kAvChunk;
    for (int m = 0; m < mc; ++m) {
      const float4 xv = xs[m][kq];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gv = gs[m][rl * 4 + r];
        acc[r].x += gv * xv.x; acc[r].y += gv * xv.y; acc[r].z += gv * xv.z; acc[r].w += gv * xv.w;
      }
    }
  }
  if (!col_ok) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = n0 + rl * 4 + r;
    if (n >= N) continue;
    const long idx = (long)n * K + k0 + kq * 4;
    adamw_update4(pv[r], acc[r], mv[r], vv[r], h);
    icl_nt_store4(p + idx, pv[r]);
    icl_nt_store4(mom + idx, mv[r]);
    icl_nt_store4(var + idx, vv[r]);
  }
}

}  // namespace icl
