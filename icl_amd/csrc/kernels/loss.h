// loss.h — fused softmax + Dice / cross-entropy / soft-Dice / MSE reductions and their gradients.
//
// Reference ops (/root/reference/code/utils/losses.py): DiceLoss :200-231 (+ CrossEntropyLoss at
// train_inherent_consistent_unet_3D_BraTS.py:107 and inside AuxLoss3D :268), softmax_dice_loss/dice_loss1
// :22-59 (PseudoSoftLoss3D), softmax_mse_loss :68-90.  The reference materialises softmax, one-hot targets
// and per-class products as full tensors (nc passes over [B,nc,S]); here one pass reads the logits (and the
// labels or the second logit tensor) and reduces every per-class sum at once; the backward is one more pass.
// HBM-bound: forward 4*nc*S (+8*S labels | +4*nc*S) bytes, backward the same + 4*nc*S written.
//
// mode 0/1 (hard target = labels): stats = [I_c = sum p_c[y==c] | Z_c = sum p_c^2 | Y_c = count(y==c) | CE = sum(lse - a_y)]
// mode 2/3 (soft target = softmax(b)): stats = [I_c = sum p_c q_c | A_c = sum p_c | Bq_c = sum q_c | MSE = sum (p-q)^2]
// out[0] = CE mean (mode 1) | MSE mean (mode 3) | 0 ;  out[1] = mean_c w_c (1 - (2I+eps)/(den+eps)), den = Z+Y | A+Bq.
#pragma once

namespace icl {

constexpr float kDiceEps = 1e-5f;

template <int NCMAX>
__device__ __forceinline__ void softmax_vec(float* v, int nc, float& lse) {
  float m = v[0];
#pragma unroll
  for (int c = 1; c < NCMAX; ++c)
    if (c < nc) m = fmaxf(m, v[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NCMAX; ++c)
    if (c < nc) { v[c] = expf(v[c] - m); s += v[c]; }
  const float inv = 1.0f / s;
#pragma unroll
  for (int c = 0; c < NCMAX; ++c)
    if (c < nc) v[c] *= inv;
  lse = m + logf(s);
}

// grid-stride over the B*S voxels; block bx of nbx writes its 3*nc+1 partial sums to part[bx][...]
template <int NCMAX>
__device__ __forceinline__ void loss_stats_body(const float* __restrict__ a, const float* __restrict__ b,
                                                const long long* __restrict__ labels, float* __restrict__ part,
                                                int B, int nc, long S, int a_is_prob, int bx, int nbx) {
  float s0[NCMAX], s1[NCMAX], s2[NCMAX];
  float sx = 0.f;
#pragma unroll
  for (int c = 0; c < NCMAX; ++c) { s0[c] = 0.f; s1[c] = 0.f; s2[c] = 0.f; }
  const long total = (long)B * S;
  for (long e = (long)bx * blockDim.x + threadIdx.x; e < total; e += (long)nbx * blockDim.x) {
    const long bi = e / S, s = e - bi * S;
    const float* ap = a + bi * nc * S + s;
    float p[NCMAX];
#pragma unroll
    for (int c = 0; c < NCMAX; ++c) p[c] = c < nc ? ap[(long)c * S] : 0.f;
    float lse = 0.f;
    if (labels) {
      const int y = (int)labels[e];
      float ay = 0.f;
#pragma unroll
      for (int c = 0; c < NCMAX; ++c)
        if (c == y) ay = p[c];
      if (!a_is_prob) { softmax_vec<NCMAX>(p, nc, lse); sx += lse - ay; }
#pragma unroll
      for (int c = 0; c < NCMAX; ++c) {
        if (c < nc) {
          const float t = (c == y) ? 1.f : 0.f;
          s0[c] += p[c] * t;
          s1[c] += p[c] * p[c];
          s2[c] += t;
        }
      }
    } else {
      const float* bp = b + bi * nc * S + s;
      float q[NCMAX];
#pragma unroll
      for (int c = 0; c < NCMAX; ++c) q[c] = c < nc ? bp[(long)c * S] : 0.f;
      float l2;
      if (!a_is_prob) softmax_vec<NCMAX>(p, nc, lse);
      softmax_vec<NCMAX>(q, nc, l2);
#pragma unroll
      for (int c = 0; c < NCMAX; ++c) {
        if (c < nc) {
          s0[c] += p[c] * q[c];
          s1[c] += p[c];
          s2[c] += q[c];
          const float d = p[c] - q[c];
          sx += d * d;
        }
      }
    }
  }
  __shared__ float red[4][3 * NCMAX + 1];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < NCMAX; ++c) {
    const float r0 = wave_sum(s0[c]), r1 = wave_sum(s1[c]), r2 = wave_sum(s2[c]);
    if (lane == 0) { red[wid][c] = r0; red[wid][NCMAX + c] = r1; red[wid][2 * NCMAX + c] = r2; }
  }
  {
    const float rx = wave_sum(sx);
    if (lane == 0) red[wid][3 * NCMAX] = rx;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 3 * NCMAX + 1) {
    const int grp = t / NCMAX, c = t - grp * NCMAX;
    if (t == 3 * NCMAX || c < nc) {
      const float v = red[0][t] + red[1][t] + red[2][t] + red[3][t];
      const int slot = (t == 3 * NCMAX) ? 3 * nc : grp * nc + c;
      part[(long)bx * (3 * nc + 1) + slot] = v;
    }
  }
}
template <int NCMAX>
__global__ __launch_bounds__(256) void loss_stats_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         const long long* __restrict__ labels, float* __restrict__ part,
                                                         int B, int nc, long S, int a_is_prob) {
  loss_stats_body<NCMAX>(a, b, labels, part, B, nc, S, a_is_prob, blockIdx.x, gridDim.x);
}

// One block: stats[slot] = sum over the nblk per-block partials in a fixed order (bit-reproducible, no atomics, nothing to
// pre-zero), then out[0], out[1] from the reduced stats.  weight may be NULL.
__device__ __forceinline__ void loss_finalize_body(const float* __restrict__ part, int nblk, float* __restrict__ stats,
                                                   const float* __restrict__ weight, float* __restrict__ out, int nc,
                                                   float inv_vox, float inv_elems, int mode) {
  // 256 threads = S slot lanes x G block groups (S = power of two >= min(nslot, 64)): thread (slot, grp) adds the partials of
  // blocks grp, grp + G, ... — a wave reads runs of consecutive floats (the slots of consecutive blocks) — and the G sums of a
  // slot are added in group order.  2 classes: 8 x 32; 16 classes: 64 x 4.  (One wave per slot with lanes over the blocks read
  // with a stride of nslot floats: 34 us for 16 classes.)
  const int nslot = 3 * nc + 1;
  __shared__ float red[256];
  int S = 8;
  while (S < nslot && S < 64) S <<= 1;
  const int G = 256 / S;
  const int sl = threadIdx.x % S, grp = threadIdx.x / S;
  for (int s0 = 0; s0 < nslot; s0 += S) {
    const int slot = s0 + sl;
    float v = 0.f;
    if (slot < nslot) {
#pragma unroll 4
      for (int b = grp; b < nblk; b += G) v += part[(long)b * nslot + slot];
    }
    __syncthreads();
    red[grp * S + sl] = v;
    __syncthreads();
    if (grp == 0 && slot < nslot) {
      float t = red[sl];
      for (int k = 1; k < G; ++k) t += red[k * S + sl];
      stats[slot] = t;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float dice = 0.f;
  for (int c = 0; c < nc; ++c) {
    const float num = 2.f * stats[c] + kDiceEps;
    const float den = stats[nc + c] + stats[2 * nc + c] + kDiceEps;
    dice += (weight ? weight[c] : 1.f) * (1.f - num / den);
  }
  out[1] = (mode == 3) ? 0.f : dice / (float)nc;
  out[0] = (mode == 1) ? stats[3 * nc] * inv_vox : (mode == 3 ? stats[3 * nc] * inv_elems : 0.f);
}
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ part, int nblk, float* __restrict__ stats,
                                                            const float* __restrict__ weight, float* __restrict__ out, int nc,
                                                            float inv_vox, float inv_elems, int mode) {
  loss_finalize_body(part, nblk, stats, weight, out, nc, inv_vox, inv_elems, mode);
}

// Per-class coefficients of the gradient, recomputed by every thread from the (3*nc+1) reduced statistics:
//   dL/dp_c(v) = alpha_c*T_c(v) + beta_c*p_c(v) + gamma_c, T = one-hot | q;  kappa scales the cross-entropy logit gradient
//   (p - t).  g0 / g1 = upstream gradients of out[0] / out[1] (NULL = that output is unused).
template <int NCMAX>
__device__ __forceinline__ void loss_grad_body(const float* __restrict__ a, const float* __restrict__ b,
                                               const long long* __restrict__ labels, const float* __restrict__ stats,
                                               const float* __restrict__ weight, const float* __restrict__ gout0,
                                               const float* __restrict__ gout1, float* __restrict__ ga, int B, int nc,
                                               long S, int mode, float inv_vox, float inv_elems, int a_is_prob, int bx, int nbx) {
  float al[NCMAX], be[NCMAX], gm[NCMAX];
  const float g0 = gout0 ? gout0[0] : 0.f, g1 = gout1 ? gout1[0] : 0.f;
#pragma unroll
  for (int c = 0; c < NCMAX; ++c) {
    al[c] = be[c] = gm[c] = 0.f;
    if (c < nc) {
      const float num = 2.f * stats[c] + kDiceEps;
      const float den = stats[nc + c] + stats[2 * nc + c] + kDiceEps;
      const float w = (weight ? weight[c] : 1.f) * g1 / (float)nc;
      if (mode == 0 || mode == 1) { al[c] = -2.f * w / den; be[c] = 2.f * w * num / (den * den); }
      else if (mode == 2) { al[c] = -2.f * w / den; gm[c] = w * num / (den * den); }
      else { al[c] = -2.f * g0 * inv_elems; be[c] = 2.f * g0 * inv_elems; }
    }
  }
  const float kappa = (mode == 1) ? g0 * inv_vox : 0.f;
  const long total = (long)B * S;
  for (long e = (long)bx * blockDim.x + threadIdx.x; e < total; e += (long)nbx * blockDim.x) {
    const long bi = e / S, s = e - bi * S;
    const float* ap = a + bi * nc * S + s;
    float* gp = ga + bi * nc * S + s;
    float p[NCMAX], T[NCMAX];
#pragma unroll
    for (int c = 0; c < NCMAX; ++c) p[c] = c < nc ? ap[(long)c * S] : 0.f;
    float lse;
    if (!a_is_prob) softmax_vec<NCMAX>(p, nc, lse);
    if (labels) {
      const int y = (int)labels[e];
#pragma unroll
      for (int c = 0; c < NCMAX; ++c) T[c] = (c == y) ? 1.f : 0.f;
    } else {
      const float* bp = b + bi * nc * S + s;
#pragma unroll
      for (int c = 0; c < NCMAX; ++c) T[c] = c < nc ? bp[(long)c * S] : 0.f;
      softmax_vec<NCMAX>(T, nc, lse);
    }
    float d[NCMAX];
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < NCMAX; ++c) {
      d[c] = c < nc ? al[c] * T[c] + be[c] * p[c] + gm[c] : 0.f;
      dot += d[c] * p[c];
    }
#pragma unroll
    for (int c = 0; c < NCMAX; ++c) {
      if (c < nc) {
        float gv = a_is_prob ? d[c] : p[c] * (d[c] - dot);
        if (labels) gv += kappa * (p[c] - T[c]);
        gp[(long)c * S] = gv;
      }
    }
  }
}
template <int NCMAX>
__global__ __launch_bounds__(256) void loss_grad_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        const long long* __restrict__ labels, const float* __restrict__ stats,
                                                        const float* __restrict__ weight, const float* __restrict__ gout0,
                                                        const float* __restrict__ gout1, float* __restrict__ ga, int B, int nc,
                                                        long S, int mode, float inv_vox, float inv_elems, int a_is_prob) {
  loss_grad_body<NCMAX>(a, b, labels, stats, weight, gout0, gout1, ga, B, nc, S, mode, inv_vox, inv_elems, a_is_prob, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------- generic-class path: 17 .. 256 classes
// The kernels above keep every class of a voxel and every per-class sum in registers (NCMAX = 4 | 16).  Here NOTHING a thread holds grows
// with nc: a thread owns one voxel of a 256-voxel tile and walks the class axis (loads coalesced along the voxel axis, class stride S) —
//   walk 1  the stable soft-max normaliser, online: running max m and sum of exp(v - m), one exp per class;
//   walk 2  p_c = exp(v_c - m) / sum and the three per-class terms of the voxel.
// The repeated walks hit the cache (a tile is 1 KB x nc).  Each term is summed over the wave (wave_sum) and lane 0 adds it to the wave's own
// row of LDS accumulators, tile after tile in a fixed order; at the end the four rows are added in wave order and written as the block's
// partials in the layout of loss_stats_body, so loss_finalize_body reduces them unchanged: no float atomics, bit-reproducible.  The tile
// loop is block-uniform (a dead lane computes on the last voxel and contributes zeros) because the wave sums sit inside it.
constexpr int kLossMaxNc = 256;

// max and sum of exp(v - max) over the nc values at p[0], p[S], ... (online: one exp per class)
__device__ __forceinline__ void softmax_norm_strided(const float* __restrict__ p, int nc, long S, float& m, float& sum) {
  m = p[0];
  sum = 1.f;
  for (int c = 1; c < nc; ++c) {
    const float v = p[(long)c * S];
    const float e = expf(-fabsf(v - m));
    sum = v > m ? sum * e + 1.f : sum + e;
    m = fmaxf(m, v);
  }
}

__device__ __forceinline__ void loss_stats_generic_body(const float* __restrict__ a, const float* __restrict__ b,
                                                        const long long* __restrict__ labels, float* __restrict__ part,
                                                        int B, int nc, long S, int a_is_prob, int bx, int nbx) {
  __shared__ float acc[4][3 * kLossMaxNc + 1];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nslot = 3 * nc + 1;
  float* my = acc[wid];
  for (int i = lane; i < nslot; i += 64) my[i] = 0.f;
  __syncthreads();
  float sx = 0.f;
  const long total = (long)B * S;
  for (long e0 = (long)bx * 256; e0 < total; e0 += (long)nbx * 256) {
    const long e = e0 + threadIdx.x;
    const bool live = e < total;
    const long ec = live ? e : total - 1;
    const long bi = ec / S, s = ec - bi * S;
    const float* ap = a + bi * nc * S + s;
    float m = 0.f, inv = 1.f;
    if (!a_is_prob) {
      float sum;
      softmax_norm_strided(ap, nc, S, m, sum);
      inv = 1.0f / sum;
      if (labels) {
        const int y = (int)labels[ec];
        const float ay = (y >= 0 && y < nc) ? ap[(long)y * S] : 0.f;
        if (live) sx += (m + logf(sum)) - ay;
      }
    }
    if (labels) {
      const int y = (int)labels[ec];
      for (int c = 0; c < nc; ++c) {
        const float v = ap[(long)c * S];
        const float p = a_is_prob ? v : expf(v - m) * inv;
        const float t = (live && c == y) ? 1.f : 0.f;
        const float r0 = wave_sum(p * t), r1 = wave_sum(live ? p * p : 0.f), r2 = wave_sum(t);
        if (lane == 0) { my[c] += r0; my[nc + c] += r1; my[2 * nc + c] += r2; }
      }
    } else {
      const float* bp = b + bi * nc * S + s;
      float m2, sum2;
      softmax_norm_strided(bp, nc, S, m2, sum2);
      const float inv2 = 1.0f / sum2;
      for (int c = 0; c < nc; ++c) {
        const float v = ap[(long)c * S];
        const float p = live ? (a_is_prob ? v : expf(v - m) * inv) : 0.f;
        const float q = live ? expf(bp[(long)c * S] - m2) * inv2 : 0.f;
        const float d = p - q;
        sx += d * d;
        const float r0 = wave_sum(p * q), r1 = wave_sum(p), r2 = wave_sum(q);
        if (lane == 0) { my[c] += r0; my[nc + c] += r1; my[2 * nc + c] += r2; }
      }
    }
  }
  {
    const float rx = wave_sum(sx);
    if (lane == 0) my[3 * nc] = rx;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nslot; t += 256)
    part[(long)bx * nslot + t] = ((acc[0][t] + acc[1][t]) + acc[2][t]) + acc[3][t];
}
__global__ __launch_bounds__(256) void loss_stats_generic_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const long long* __restrict__ labels, float* __restrict__ part,
                                                                 int B, int nc, long S, int a_is_prob) {
  loss_stats_generic_body(a, b, labels, part, B, nc, S, a_is_prob, blockIdx.x, gridDim.x);
}

// The gradient of loss_grad_body with the per-class coefficients in LDS (3 x 256 floats, computed once per block) and three walks over
// the classes of a voxel: the normaliser(s), dot = sum_c d_c p_c (soft-max inputs only), the gradient itself.
__device__ __forceinline__ void loss_grad_generic_body(const float* __restrict__ a, const float* __restrict__ b,
                                                       const long long* __restrict__ labels, const float* __restrict__ stats,
                                                       const float* __restrict__ weight, const float* __restrict__ gout0,
                                                       const float* __restrict__ gout1, float* __restrict__ ga, int B, int nc,
                                                       long S, int mode, float inv_vox, float inv_elems, int a_is_prob, int bx, int nbx) {
  __shared__ float al[kLossMaxNc], be[kLossMaxNc], gm[kLossMaxNc];
  const float g0 = gout0 ? gout0[0] : 0.f, g1 = gout1 ? gout1[0] : 0.f;
  for (int c = threadIdx.x; c < nc; c += 256) {
    const float num = 2.f * stats[c] + kDiceEps;
    const float den = stats[nc + c] + stats[2 * nc + c] + kDiceEps;
    const float w = (weight ? weight[c] : 1.f) * g1 / (float)nc;
    float x = 0.f, y = 0.f, z = 0.f;
    if (mode == 0 || mode == 1) { x = -2.f * w / den; y = 2.f * w * num / (den * den); }
    else if (mode == 2) { x = -2.f * w / den; z = w * num / (den * den); }
    else { x = -2.f * g0 * inv_elems; y = 2.f * g0 * inv_elems; }
    al[c] = x; be[c] = y; gm[c] = z;
  }
  __syncthreads();
  const float kappa = (mode == 1) ? g0 * inv_vox : 0.f;
  const long total = (long)B * S;
  for (long e = (long)bx * 256 + threadIdx.x; e < total; e += (long)nbx * 256) {
    const long bi = e / S, s = e - bi * S;
    const float* ap = a + bi * nc * S + s;
    float* gp = ga + bi * nc * S + s;
    float m = 0.f, inv = 1.f;
    if (!a_is_prob) {
      float sum;
      softmax_norm_strided(ap, nc, S, m, sum);
      inv = 1.0f / sum;
    }
    if (labels) {
      const int y = (int)labels[e];
      float dot = 0.f;
      if (!a_is_prob) {
        for (int c = 0; c < nc; ++c) {
          const float p = expf(ap[(long)c * S] - m) * inv;
          dot += ((c == y ? al[c] : 0.f) + be[c] * p + gm[c]) * p;
        }
      }
      for (int c = 0; c < nc; ++c) {
        const float v = ap[(long)c * S];
        const float p = a_is_prob ? v : expf(v - m) * inv;
        const float T = (c == y) ? 1.f : 0.f;
        const float d = al[c] * T + be[c] * p + gm[c];
        gp[(long)c * S] = (a_is_prob ? d : p * (d - dot)) + kappa * (p - T);
      }
    } else {
      const float* bp = b + bi * nc * S + s;
      float m2, sum2;
      softmax_norm_strided(bp, nc, S, m2, sum2);
      const float inv2 = 1.0f / sum2;
      float dot = 0.f;
      if (!a_is_prob) {
        for (int c = 0; c < nc; ++c) {
          const float p = expf(ap[(long)c * S] - m) * inv;
          const float T = expf(bp[(long)c * S] - m2) * inv2;
          dot += (al[c] * T + be[c] * p + gm[c]) * p;
        }
      }
      for (int c = 0; c < nc; ++c) {
        const float v = ap[(long)c * S];
        const float p = a_is_prob ? v : expf(v - m) * inv;
        const float T = expf(bp[(long)c * S] - m2) * inv2;
        const float d = al[c] * T + be[c] * p + gm[c];
        gp[(long)c * S] = a_is_prob ? d : p * (d - dot);
      }
    }
  }
}
__global__ __launch_bounds__(256) void loss_grad_generic_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                const long long* __restrict__ labels, const float* __restrict__ stats,
                                                                const float* __restrict__ weight, const float* __restrict__ gout0,
                                                                const float* __restrict__ gout1, float* __restrict__ ga, int B, int nc,
                                                                long S, int mode, float inv_vox, float inv_elems, int a_is_prob) {
  loss_grad_generic_body(a, b, labels, stats, weight, gout0, gout1, ga, B, nc, S, mode, inv_vox, inv_elems, a_is_prob, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------- all loss terms of a step in one launch per pass (round 6)
// The five-part objective of the trainer (:105-112) is ten reductions — CE + Dice on the logits, three AuxLoss3D maps, three
// PseudoSoftLoss3D maps, three softmax-MSE pairs — each a statistics launch and a one-block finalize, one behind the other on the step's
// stream with nothing beside them (0.2 ms of 5-10 us launches), and ten gradient launches at the head of the backward pass.  Job j of
// these kernels IS launch j of the single-term kernels (same blocks, same partial sums, same order: bit-identical); grid (blocks, jobs).
constexpr int kLossMulti = 12;
struct LossMulti {
  const float* a[kLossMulti]; const float* b[kLossMulti]; const long long* lab[kLossMulti]; const float* weight[kLossMulti];
  float* stats[kLossMulti]; float* out[kLossMulti];
  const float* g0[kLossMulti]; const float* g1[kLossMulti]; float* ga[kLossMulti];
  long S[kLossMulti];
  int B[kLossMulti], nc[kLossMulti], mode[kLossMulti], aip[kLossMulti], nblk[kLossMulti];
};
template <int NCMAX>
__global__ __launch_bounds__(256) void loss_stats_multi_kernel(LossMulti m) {
  const int j = blockIdx.y;
  if ((int)blockIdx.x >= m.nblk[j]) return;
  loss_stats_body<NCMAX>(m.a[j], m.b[j], m.lab[j], m.stats[j] + (3 * m.nc[j] + 1), m.B[j], m.nc[j], m.S[j], m.aip[j], blockIdx.x, m.nblk[j]);
}
__global__ __launch_bounds__(256) void loss_finalize_multi_kernel(LossMulti m) {
  const int j = blockIdx.x;
  const float total = (float)((long)m.B[j] * m.S[j]);
  loss_finalize_body(m.stats[j] + (3 * m.nc[j] + 1), m.nblk[j], m.stats[j], m.weight[j], m.out[j], m.nc[j], 1.0f / total,
                     1.0f / (total * (float)m.nc[j]), m.mode[j]);
}
template <int NCMAX>
__global__ __launch_bounds__(256) void loss_grad_multi_kernel(LossMulti m) {
  const int j = blockIdx.y;
  if ((int)blockIdx.x >= m.nblk[j]) return;
  const float total = (float)((long)m.B[j] * m.S[j]);
  loss_grad_body<NCMAX>(m.a[j], m.b[j], m.lab[j], m.stats[j], m.weight[j], m.g0[j], m.g1[j], m.ga[j], m.B[j], m.nc[j], m.S[j], m.mode[j],
                        1.0f / total, 1.0f / (total * (float)m.nc[j]), m.aip[j], blockIdx.x, m.nblk[j]);
}

__global__ __launch_bounds__(256) void loss_stats_generic_multi_kernel(LossMulti m) {
  const int j = blockIdx.y;
  if ((int)blockIdx.x >= m.nblk[j]) return;
  loss_stats_generic_body(m.a[j], m.b[j], m.lab[j], m.stats[j] + (3 * m.nc[j] + 1), m.B[j], m.nc[j], m.S[j], m.aip[j], blockIdx.x, m.nblk[j]);
}
__global__ __launch_bounds__(256) void loss_grad_generic_multi_kernel(LossMulti m) {
  const int j = blockIdx.y;
  if ((int)blockIdx.x >= m.nblk[j]) return;
  const float total = (float)((long)m.B[j] * m.S[j]);
  loss_grad_generic_body(m.a[j], m.b[j], m.lab[j], m.stats[j], m.weight[j], m.g0[j], m.g1[j], m.ga[j], m.B[j], m.nc[j], m.S[j], m.mode[j],
                         1.0f / total, 1.0f / (total * (float)m.nc[j]), m.aip[j], blockIdx.x, m.nblk[j]);
}

}  // namespace icl
