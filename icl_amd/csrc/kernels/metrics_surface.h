// metrics_surface.h — surface metrics with a voxel spacing, every foreground class, on the device: HD95, HD, ASD / ASSD and the voxel-border
// NSD in the spacing's units (the reference calls medpy.metric.binary.hd95 without `voxelspacing`; MedPy's hd95 / hd / asd / assd take it:
// restated in icl_amd/val_3D.py binary_hd95 / binary_hd / binary_asd / binary_assd / binary_nsd).  This is the floating-point path BESIDE
// the integer one of metrics.h, which stays as it is: with a spacing (s0, s1, s2) the squared distance is the double
// sum_a ((double)delta_a * s_a)^2, so there is no integer to index a histogram with.  Per class c in 1..C-1 the kernels return
//   counts[7] = {|P|, |G|, |P & G|, |dP|, |dG|, #{p in dP: d(p, dG) <= tau}, #{g in dG: d(g, dP) <= tau}}          (integers)
//   values[6] = {sq[k0], sq[k0 + 1], max d^2 (P -> G), max d^2 (G -> P), sum d (P -> G), sum d (G -> P)}           (doubles; -1 when dP or dG is empty)
// with sq the sorted union of the squared distances of both directions and k0 = floor(0.95 (n - 1)), n = |dP| + |dG| (metrics.h).
//
// Passes (V = n0 n1 n2 voxels):
//   1. seg_border_kernel, seg_bbox_kernel of metrics.h, unchanged: border byte maps, counters, the boxes of dP and dG.
//   2. Per class and direction (F the feature set's box, Q the query set's, as in metrics.h) the weighted exact distance transform in
//      double: surf_edt_axis2_kernel on F0 x F1 x Q2, surf_edt_axis1_kernel on F0 x Q1 x Q2, surf_edt_axis0_kernel at the query border
//      voxels of Q.  An axis term is t = (double)delta * s_a; t * t (multiply, then square, as scipy forms it); a pass adds its term to
//      the value of the pass before; contraction is off, so every product and sum is rounded on its own.  The outward scan stops once the
//      term alone is >= the best sum so far: exact, because rounding is monotone (a farther term is no smaller, and adding a non-negative
//      value to it gives no less).  Lines without a feature hold +infinity.  The axis-0 pass writes the squared distance of every query border
//      voxel into a dense Q-box-shaped buffer, kSurfNone (-1) elsewhere; one buffer per direction, both live until the class is done.
//   3. surf_reduce_kernel, one launch per direction over the dense buffer: max d^2, sum of sqrt(d^2) and the count of d^2 <= tau^2, each
//      thread over its grid-stride elements in index order, then a fixed tree over the workgroup, one partial per workgroup; the last
//      kernel adds the partials in index order.  No floating-point atomics: two runs are bit-equal.
//   4. Order statistics by a most-significant-digit radix select over the union of the two buffers: a non-negative double orders as its
//      bit pattern.  kSurfPasses passes of kSurfDigitBits bits (6 x 11 >= 63).  surf_radix_kernel<PASS> counts the digit of every key
//      that carries the prefix of rank k0 (histogram A) or of rank k0 + 1 (histogram B; only when the two prefixes differ — the ranks may
//      leave each other's bucket at any digit): LDS integer atomics, then one global integer atomic per non-empty bin.  The prefixes and
//      the ranks inside their buckets after pass p are a function of the histograms 0..p alone; every workgroup of pass p + 1 advances
//      them from the state after pass p - 1 (surf_advance; workgroup 0 stores the state for the pass after) — no launch in between.
//      surf_finish_kernel advances once more, writes the record and clears the histograms for the next class.
// Launches per class: 6 (transform) + 2 (reduce) + 6 (radix) + 1 = 15, all on the caller's stream, no synchronisation.
// Workspace: 2 bytes per voxel of border maps + 4 x 8 bytes per voxel (two transform buffers, two dense buffers) = 34 bytes per voxel,
// plus counters, flags, boxes, 96 KiB of histograms and the partials.
#pragma once

namespace icl {

constexpr int kSurfThreads = 256;
constexpr int kSurfDigitBits = 11;
constexpr int kSurfBins = 1 << kSurfDigitBits;
constexpr int kSurfPasses = 6;                 // digit p covers bits [shift, shift + 11), shift = 11 (5 - p); the top digit holds bits 55..63
constexpr int kSurfMaxParts = 1024;            // workgroups of surf_reduce_kernel
constexpr int kSurfCounts = 7, kSurfValues = 6;
constexpr double kSurfNone = -1.0;             // dense buffer: not a query border voxel (real squared distances are >= 0)

// prefix (the digits chosen so far, lower bits zero) and rank inside the bucket, for k0 (a) and k0 + 1 (b)
struct SurfSel {
  unsigned long long pa, pb;
  long long ra, rb;
};

__device__ __forceinline__ double surf_inf() { return __builtin_huge_val(); }

__device__ __forceinline__ unsigned long long surf_key(double v) {
  unsigned long long u;
  __builtin_memcpy(&u, &v, 8);
  return u;
}

__device__ __forceinline__ double surf_from_key(unsigned long long u) {
  double v;
  __builtin_memcpy(&v, &u, 8);
  return v;
}

// (delta * s)^2: the product first, then the square, each rounded on its own
__device__ __forceinline__ double surf_term(int delta, double s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double t = (double)delta * s;
  return t * t;
}

__device__ __forceinline__ double surf_sum(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a + b;
}

// Pass along axis 2 on F0 x F1 x Q2: d[e] = ((z - f) s2)^2 for the nearest feature f of the line, +infinity without one.  d: [fe0][fe1][qe2].
__global__ __launch_bounds__(256) void surf_edt_axis2_kernel(const unsigned char* __restrict__ feat, const int* __restrict__ box,
                                                             double* __restrict__ d, int k, int dir, int n1, int n2, double s2) {
  SegDir g;
  if (!seg_load_dir(box, k, dir, g)) return;
  const long nb = (long)g.fe0 * g.fe1 * g.qe2;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nb; e += (long)gridDim.x * blockDim.x) {
    const int z = g.q2 + (int)(e % g.qe2);
    const long r = e / g.qe2;
    const int y = g.f1 + (int)(r % g.fe1), x = g.f0 + (int)(r / g.fe1);
    const unsigned char* line = feat + ((long)x * n1 + y) * n2;
    const int lo = g.f2, hi = g.f2 + g.fe2 - 1;
    double best = surf_inf();
    for (int s = seg_gap(z, lo, g.fe2);; ++s) {
      const int a = z - s, c = z + s;
      if (a < lo && c > hi) break;
      if ((a >= lo && a <= hi && line[a] == k) || (c >= lo && c <= hi && line[c] == k)) {
        best = surf_term(s, s2);
        break;
      }
    }
    d[e] = best;
  }
}

// min over u' in [lo, hi] of ((u - u') s)^2 + line[(u' - lo) * stride]: the pruned outward scan of metrics.h in double
__device__ __forceinline__ double surf_scan(const double* line, long stride, int u, int lo, int ext, double s) {
  const int hi = lo + ext - 1;
  double best = surf_inf();
  for (int o = seg_gap(u, lo, ext);; ++o) {
    const double t = surf_term(o, s);
    const int a = u - o, c = u + o;
    if (t >= best || (a < lo && c > hi)) break;
    if (a >= lo && a <= hi) {
      const double v = surf_sum(line[(long)(a - lo) * stride], t);      // +infinity stays +infinity
      if (v < best) best = v;
    }
    if (o > 0 && c >= lo && c <= hi) {
      const double v = surf_sum(line[(long)(c - lo) * stride], t);
      if (v < best) best = v;
    }
  }
  return best;
}

// Pass along axis 1 on F0 x Q1 x Q2.  in: [fe0][fe1][qe2], out: [fe0][qe1][qe2].
__global__ __launch_bounds__(256) void surf_edt_axis1_kernel(const double* __restrict__ in, const int* __restrict__ box, double* __restrict__ out,
                                                             int k, int dir, double s1) {
  SegDir g;
  if (!seg_load_dir(box, k, dir, g)) return;
  const long nb = (long)g.fe0 * g.qe1 * g.qe2;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nb; e += (long)gridDim.x * blockDim.x) {
    const int iz = (int)(e % g.qe2);
    const long r = e / g.qe2;
    const int y = g.q1 + (int)(r % g.qe1), ix = (int)(r / g.qe1);
    out[e] = surf_scan(in + (long)ix * g.fe1 * g.qe2 + iz, g.qe2, y, g.f1, g.fe1, s1);
  }
}

// Pass along axis 0 over Q.  in: [fe0][qe1][qe2]; dense: [qe0][qe1][qe2], the squared distance at the voxels whose QUERY border byte is k,
// kSurfNone elsewhere.
__global__ __launch_bounds__(256) void surf_edt_axis0_kernel(const double* __restrict__ in, const unsigned char* __restrict__ query,
                                                             const int* __restrict__ box, double* __restrict__ dense, int k, int dir, int n1,
                                                             int n2, double s0) {
  SegDir g;
  if (!seg_load_dir(box, k, dir, g)) return;
  const long plane = (long)g.qe1 * g.qe2, nb = (long)g.qe0 * plane;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nb; e += (long)gridDim.x * blockDim.x) {
    const int iz = (int)(e % g.qe2);
    const long r = e / g.qe2;
    const int iy = (int)(r % g.qe1), x = g.q0 + (int)(r / g.qe1);
    double v = kSurfNone;
    if (query[((long)x * n1 + (g.q1 + iy)) * n2 + g.q2 + iz] == k) v = surf_scan(in + (long)iy * g.qe2 + iz, plane, x, g.f0, g.fe0, s0);
    dense[e] = v;
  }
}

// One direction's dense buffer -> one partial per workgroup: psum / pmax [gridDim.x] doubles, pcnt [gridDim.x].  tau2 = tolerance^2.
__global__ __launch_bounds__(kSurfThreads) void surf_reduce_kernel(const double* __restrict__ dense, const int* __restrict__ box,
                                                                    double* __restrict__ psum, double* __restrict__ pmax,
                                                                    unsigned* __restrict__ pcnt, int k, int dir, double tau2) {
  __shared__ double ls[kSurfThreads];
  __shared__ double lm[kSurfThreads];
  __shared__ unsigned lc[kSurfThreads];
  SegDir g;
  if (!seg_load_dir(box, k, dir, g)) return;      // uniform over the launch
  const long nb = (long)g.qe0 * g.qe1 * g.qe2;
  double s = 0.0, m = kSurfNone;
  unsigned c = 0u;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nb; e += (long)gridDim.x * blockDim.x) {
    const double v = dense[e];
    if (v < 0.0) continue;
    s = surf_sum(s, sqrt(v));
    if (v > m) m = v;
    if (v <= tau2) ++c;
  }
  ls[threadIdx.x] = s;
  lm[threadIdx.x] = m;
  lc[threadIdx.x] = c;
  __syncthreads();
  for (int w = kSurfThreads / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) {
      ls[threadIdx.x] = surf_sum(ls[threadIdx.x], ls[threadIdx.x + w]);
      if (lm[threadIdx.x + w] > lm[threadIdx.x]) lm[threadIdx.x] = lm[threadIdx.x + w];
      lc[threadIdx.x] += lc[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    psum[blockIdx.x] = ls[0];
    pmax[blockIdx.x] = lm[0];
    pcnt[blockIdx.x] = lc[0];
  }
}

__device__ __forceinline__ SurfSel surf_initial(const unsigned* cnt, int k) {
  const long long n = (long long)cnt[k * kSegCnt + 3] + (long long)cnt[k * kSegCnt + 4];
  // numpy's `linear` percentile: virtual index (n - 1) * 0.95 in double (one rounding), its floor and the next rank (seg_select_kernel)
  const long long k0 = (long long)((double)(n - 1) * 0.95);
  SurfSel s;
  s.pa = s.pb = 0ull;
  s.ra = k0;
  s.rb = k0 + 1;
  return s;
}

// the bin of `h` [kSurfBins] that holds rank r, and r's rank inside it.  All kSurfThreads threads call it; part [kSurfThreads], res [2].
__device__ __forceinline__ void surf_pick(const unsigned* h, long long r, unsigned long long* part, long long* res) {
  constexpr int per = kSurfBins / kSurfThreads;
  unsigned long long s = 0;
  for (int i = 0; i < per; ++i) s += h[threadIdx.x * per + i];
  part[threadIdx.x] = s;
  if (threadIdx.x == 0) res[0] = -1;
  __syncthreads();
  if (threadIdx.x == 0) {      // exclusive prefix over the chunk sums
    unsigned long long run = 0;
    for (int t = 0; t < kSurfThreads; ++t) {
      const unsigned long long v = part[t];
      part[t] = run;
      run += v;
    }
  }
  __syncthreads();
  const long long first = (long long)part[threadIdx.x];
  if (r >= first && r < first + (long long)s) {      // exactly one thread when the rank lies in the histogram
    long long run = first;
    for (int i = 0; i < per; ++i) {
      const long long c = h[threadIdx.x * per + i];
      if (r >= run && r < run + c) {
        res[0] = threadIdx.x * per + i;
        res[1] = r - run;
      }
      run += c;
    }
  }
  __syncthreads();
}

// the state after the pass whose histograms are ha (prefix pa) and hb (prefix pb, counted only when pb != pa), from the state before it
__device__ __forceinline__ SurfSel surf_advance(SurfSel s, const unsigned* ha, const unsigned* hb, int shift, unsigned long long* part,
                                                long long* res) {
  const bool same = s.pa == s.pb;
  SurfSel o = s;
  surf_pick(ha, s.ra, part, res);
  if (res[0] >= 0) {
    o.pa = s.pa | ((unsigned long long)res[0] << shift);
    o.ra = res[1];
  }
  __syncthreads();      // res is read by every thread before the next pick rewrites it
  surf_pick(same ? ha : hb, s.rb, part, res);
  if (res[0] >= 0) {
    o.pb = s.pb | ((unsigned long long)res[0] << shift);
    o.rb = res[1];
  }
  __syncthreads();
  return o;
}

constexpr int surf_shift(int pass) { return kSurfDigitBits * (kSurfPasses - 1 - pass); }
// the bits above the digit of `pass` (none in pass 0: 6 x 11 > 64)
constexpr unsigned long long surf_above(int pass) { return pass == 0 ? 0ull : ~0ull << (surf_shift(pass) + kSurfDigitBits); }

// Pass PASS of the select.  hist: [kSurfPasses][2][kSurfBins], zero before the class's first pass; state: [kSurfPasses] (slot p: after pass p).
// da / db: the dense buffers of direction 0 (Q = the box of dP) and 1 (Q = the box of dG).
template <int PASS>
__global__ __launch_bounds__(kSurfThreads) void surf_radix_kernel(const double* __restrict__ da, const double* __restrict__ db,
                                                                   const unsigned* __restrict__ cnt, const int* __restrict__ box,
                                                                   unsigned* __restrict__ hist, SurfSel* __restrict__ state, int k) {
  __shared__ unsigned lh[2 * kSurfBins];
  __shared__ unsigned long long part[kSurfThreads];
  __shared__ long long res[2];
  SegDir g;
  if (!seg_load_dir(box, k, 0, g)) return;      // uniform over the launch: no barrier is skipped by part of a workgroup
  SurfSel s = surf_initial(cnt, k);
  if constexpr (PASS >= 1) {
    if constexpr (PASS >= 2) s = state[PASS - 2];
    const unsigned* hp = hist + (long)(PASS - 1) * 2 * kSurfBins;
    s = surf_advance(s, hp, hp + kSurfBins, surf_shift(PASS - 1), part, res);
    if (blockIdx.x == 0 && threadIdx.x == 0) state[PASS - 1] = s;
  }
  for (int i = threadIdx.x; i < 2 * kSurfBins; i += blockDim.x) lh[i] = 0u;
  __syncthreads();
  constexpr int shift = surf_shift(PASS);
  constexpr unsigned long long above = surf_above(PASS);
  const bool same = s.pa == s.pb;
  const long na = (long)g.qe0 * g.qe1 * g.qe2, nb = (long)g.fe0 * g.fe1 * g.fe2;      // direction 1 queries the box that direction 0 calls F
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < na + nb; e += (long)gridDim.x * blockDim.x) {
    const double v = e < na ? da[e] : db[e - na];
    if (v < 0.0) continue;
    const unsigned long long key = surf_key(v);
    const int digit = (int)((key >> shift) & (unsigned long long)(kSurfBins - 1));
    if ((key & above) == s.pa) atomicAdd(&lh[digit], 1u);
    if (!same && (key & above) == s.pb) atomicAdd(&lh[kSurfBins + digit], 1u);
  }
  __syncthreads();
  unsigned* h = hist + (long)PASS * 2 * kSurfBins;
  for (int i = threadIdx.x; i < 2 * kSurfBins; i += blockDim.x)
    if (lh[i]) atomicAdd(&h[i], lh[i]);
}

// One workgroup: the records of class k (row k - 1 of counts / values); for a valid class the last digit of the select and the partials of
// both directions (`parts` workgroups each; psum / pmax / pcnt: [2][kSurfMaxParts]), added in index order.  Clears the histograms.
__global__ __launch_bounds__(kSurfThreads) void surf_finish_kernel(const unsigned* __restrict__ cnt, const int* __restrict__ box,
                                                                    unsigned* __restrict__ hist, const SurfSel* __restrict__ state,
                                                                    const double* __restrict__ psum, const double* __restrict__ pmax,
                                                                    const unsigned* __restrict__ pcnt, int parts, long long* __restrict__ counts,
                                                                    double* __restrict__ values, int k) {
  __shared__ unsigned long long part[kSurfThreads];
  __shared__ long long res[2];
  const unsigned* c = cnt + k * kSegCnt;
  long long* rc = counts + (long)(k - 1) * kSurfCounts;
  double* rv = values + (long)(k - 1) * kSurfValues;
  SegDir g;
  const bool valid = seg_load_dir(box, k, 0, g);
  if (threadIdx.x == 0) {
    for (int i = 0; i < kSegCnt; ++i) rc[i] = c[i];
    rc[5] = rc[6] = 0;
    for (int i = 0; i < kSurfValues; ++i) rv[i] = -1.0;
  }
  if (!valid) return;      // uniform over the workgroup; the histograms of an invalid class were never written
  const unsigned* hp = hist + (long)(kSurfPasses - 1) * 2 * kSurfBins;
  const SurfSel s = surf_advance(state[kSurfPasses - 2], hp, hp + kSurfBins, 0, part, res);
  if (threadIdx.x == 0) {
    rv[0] = surf_from_key(s.pa);
    rv[1] = surf_from_key(s.pb);
    for (int dir = 0; dir < 2; ++dir) {
      double sum = 0.0, mx = kSurfNone;
      long long within = 0;
      for (int i = 0; i < parts; ++i) {
        sum = surf_sum(sum, psum[dir * kSurfMaxParts + i]);
        const double m = pmax[dir * kSurfMaxParts + i];
        if (m > mx) mx = m;
        within += pcnt[dir * kSurfMaxParts + i];
      }
      rv[2 + dir] = mx;
      rv[4 + dir] = sum;
      rc[5 + dir] = within;
    }
  }
  for (int i = threadIdx.x; i < kSurfPasses * 2 * kSurfBins; i += blockDim.x) hist[i] = 0u;
}

}  // namespace icl
