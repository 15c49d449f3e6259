// components.h — connected components of a label map on the device, every foreground class in ONE labelling, and the keep-largest /
// minimum-size filter that validation pipelines apply between the arg-max and the scores (scipy.ndimage.label once per class on the
// host; restated in icl_amd/val_3D.py keep_components).  Class rule: seg_class of metrics.h.  Two neighbouring voxels are joined only
// when they carry the same class, so the number of launches does not depend on num_classes.  CONN = 1 / 2 / 3: 6 / 18 / 26 neighbours
// (scipy.ndimage.generate_binary_structure(3, CONN)); a neighbour outside the volume does not exist.
//
// Result: labels[v] = 0 on background, else 1 + (linear index of the first voxel, in raster order, of v's component) — a function of
// the map alone, whatever the schedule.  Everything is integer: two runs are bit-equal.
//
// Passes (V = n0 n1 n2 voxels; `parent` holds, for a foreground voxel, the linear index of a voxel of its component that is not
// later in raster order — a root points at itself — and -1 on background):
//   1. cc_tile_kernel: one workgroup labels a kCcT0 x kCcT1 x kCcT2 tile (with a rim of class 0) in LDS to a fixed point (label
//      equivalence: every voxel hooks its root under the smallest root among its neighbours with an LDS atomic min, then every voxel
//      jumps to its root; repeated until nothing changes).  Local order = raster order inside a tile, so a tile component's root is its first voxel.  Writes parent and
//      size (the component's voxel count inside the tile at its tile root, 0 elsewhere).
//   2. cc_merge_kernel: every voxel looks at the neighbours of CONN that come before it in raster order and lie in ANOTHER tile — the tile
//      faces, edges and corners that CONN joins — and unites the two trees: find both roots, atomic min on the larger root with the
//      smaller, and where the returned value says that root had a parent already, go on with that parent (cc_unite).  parent is written
//      by many workgroups here, so EVERY access to it in this kernel is an agent-scope atomic (cc_load, cc_min); the loop follows the
//      value the atomic returns, never a re-read.  No workgroup waits for another: every step of find moves to a strictly smaller
//      index, every retry of unite starts from a strictly smaller one.
//   3. cc_flatten_kernel: parent is read-only now (plain loads across the kernel boundary): labels[v] = 1 + root(v); every tile root
//      that is not its component's root adds its tile count to the root's slot of size (integer atomic: order-free).
//   4. cc_reduce_kernel: the roots (labels[v] == v + 1) by class: number of components and the maximum of the key
//      (size << 32) | (2^31 - 1 - v) — the larger component wins, among equals the one that starts first (np.argmax over scipy's sizes);
//      a maximum does not depend on the order.  One partial per workgroup and class; cc_finish_kernel (one workgroup) combines them in
//      index order and writes the per-class record {components, voxels in the largest, label of the largest}.
//   5. cc_filter_kernel: out[v] = class of v if its component is kept, else 0 (labels outside 1..num_classes-1 are background: 0).
// 5 launches for the labelling, 6 with the filter, whatever the data.  Workspace: 8 bytes per voxel (parent, size) for the labelling,
// 12 with the filter (its labels), plus the partials.
#pragma once

namespace icl {

constexpr int kCcT0 = 8, kCcT1 = 8, kCcT2 = 16;      // tile extents along axes 0, 1, 2
constexpr int kCcTile = kCcT0 * kCcT1 * kCcT2;
constexpr int kCcThreads = 256;
constexpr int kCcPer = kCcTile / kCcThreads;         // voxels of a tile per thread
constexpr int kCcS1 = kCcT2 + 2, kCcS0 = (kCcT1 + 2) * kCcS1;      // strides of the tile with its rim in LDS
constexpr int kCcCells = (kCcT0 + 2) * kCcS0;
constexpr int kCcMaxParts = 256;                     // workgroups of cc_reduce_kernel
constexpr int kCcRec = 3;                            // per-class record: components, voxels in the largest, its label
constexpr int kCcIdxMax = 0x7fffffff;

// The atomics nothing else in the project needs.  Agent scope for words that several workgroups write in one launch (the loads and the
// min go to the device-coherent level, past this CU's L1); workgroup scope for LDS.
#if defined(__HIPCC__)
__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_lds_min(int* p, int v) {
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void cc_lds_max64(unsigned long long* p, unsigned long long v) {
  __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
#else
inline int cc_load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
inline int cc_min(int* p, int v) {
  int old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
  return old;
}
inline int cc_lds_min(int* p, int v) { return cc_min(p, v); }
inline void cc_lds_max64(unsigned long long* p, unsigned long long v) {
  unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v > old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
}
#endif

// is (da, db, dc) != 0 a neighbour offset of connectivity CONN?
template <int CONN>
__device__ __forceinline__ constexpr bool cc_joined(int da, int db, int dc) {
  const int nz = (da != 0) + (db != 0) + (dc != 0);
  return nz >= 1 && nz <= CONN;
}

// voxel i of the tile -> its cell in the rimmed tile
__device__ __forceinline__ int cc_cell(int i) {
  return (i / (kCcT1 * kCcT2) + 1) * kCcS0 + ((i / kCcT2) % kCcT1 + 1) * kCcS1 + i % kCcT2 + 1;
}

// Pass 1.  Grid: one workgroup per tile, tile t = (t0 nt1 + t1) nt2 + t2.  The tile sits in LDS with a one-voxel rim of class 0 (also
// the voxels past the volume's end carry class 0), so a neighbour needs no bounds check; a label is a cell index of the rimmed tile,
// which orders the tile's voxels as the raster does.
template <typename T, int CONN>
__global__ __launch_bounds__(kCcThreads) void cc_tile_kernel(const T* __restrict__ map, int* __restrict__ parent, int* __restrict__ size,
                                                             int n0, int n1, int n2, int nc, int nt1, int nt2) {
  __shared__ int lab[kCcCells];
  __shared__ int cnt[kCcCells];
  __shared__ unsigned char cls[kCcCells];
  __shared__ int changed;
  const int t2 = (int)(blockIdx.x % nt2), t1 = (int)((blockIdx.x / nt2) % nt1), t0 = (int)(blockIdx.x / ((long)nt1 * nt2));
  const int a0 = t0 * kCcT0, b0 = t1 * kCcT1, c0 = t2 * kCcT2;
  for (int p = threadIdx.x; p < kCcCells; p += kCcThreads) {
    cls[p] = 0;
    lab[p] = p;
    cnt[p] = 0;
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < kCcPer; ++k) {
    const int i = threadIdx.x + k * kCcThreads;
    const int a = a0 + i / (kCcT1 * kCcT2), b = b0 + (i / kCcT2) % kCcT1, c = c0 + i % kCcT2;
    if (a < n0 && b < n1 && c < n2) cls[cc_cell(i)] = (unsigned char)seg_class(map, ((long)a * n1 + b) * n2 + c, nc);
  }
  for (;;) {
    __syncthreads();      // classes / the labels of the round before are in place; every thread has read `changed`
    if (threadIdx.x == 0) changed = 0;
    __syncthreads();
    // hook: at this point every label is a root (lab[l] == l).  The root of a voxel goes under the smallest root next to the voxel.
#pragma unroll 1
    for (int k = 0; k < kCcPer; ++k) {
      const int p = cc_cell(threadIdx.x + k * kCcThreads);
      const int q = cls[p];
      if (!q) continue;
      const int l = lab[p];
      int m = l;
#pragma unroll
      for (int da = -1; da <= 1; ++da)
#pragma unroll
        for (int db = -1; db <= 1; ++db)
#pragma unroll
          for (int dc = -1; dc <= 1; ++dc) {
            if (!cc_joined<CONN>(da, db, dc)) continue;
            const int j = p + da * kCcS0 + db * kCcS1 + dc;
            const int v = lab[j];
            if (cls[j] == q && v < m) m = v;
          }
      if (m < l) {
        cc_lds_min(&lab[l], m);
        changed = 1;
      }
    }
    __syncthreads();
    // jump: the chain from a voxel strictly decreases and ends at a root; roots do not change in this phase
#pragma unroll 1
    for (int k = 0; k < kCcPer; ++k) {
      const int p = cc_cell(threadIdx.x + k * kCcThreads);
      if (!cls[p]) continue;
      int l = lab[p];
      for (int up = lab[l]; up != l; up = lab[l]) l = up;
      lab[p] = l;
    }
    if (!changed) break;      // uniform: written before the barrier above, cleared after the next one
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < kCcPer; ++k) {
    const int p = cc_cell(threadIdx.x + k * kCcThreads);
    if (cls[p]) atomicAdd(&cnt[lab[p]], 1);
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < kCcPer; ++k) {
    const int i = threadIdx.x + k * kCcThreads;
    const int a = a0 + i / (kCcT1 * kCcT2), b = b0 + (i / kCcT2) % kCcT1, c = c0 + i % kCcT2;
    if (a >= n0 || b >= n1 || c >= n2) continue;
    const long e = ((long)a * n1 + b) * n2 + c;
    const int p = cc_cell(i);
    int r = -1;
    if (cls[p]) {
      const int l = lab[p];      // a cell inside the rim: coordinates in the tile are the cell's minus one
      r = (int)(((long)(a0 + l / kCcS0 - 1) * n1 + b0 + (l / kCcS1) % (kCcT1 + 2) - 1) * n2 + c0 + l % kCcS1 - 1);
    }
    parent[e] = r;
    size[e] = cnt[p];      // 0 unless this voxel is a tile root
  }
}

// The root of x as far as this thread can see it; every step goes to a strictly smaller index.
__device__ __forceinline__ int cc_find(const int* parent, int x) {
  for (int p = cc_load(&parent[x]); p != x; p = cc_load(&parent[x])) x = p;
  return x;
}

// Unite the trees of x and y.  The min returns what the larger root's word held: itself — it was a root and now hangs under the smaller
// one, done; anything else `old` < x — x had a parent already, and the word now holds min(old, y), so the edge x -> old may be gone:
// uniting old and y restores it (and is what is left to do in the other cases too).
__device__ __forceinline__ void cc_unite(int* parent, int x, int y) {
  for (;;) {
    x = cc_find(parent, x);
    y = cc_find(parent, y);
    if (x == y) return;
    if (x < y) {
      const int t = x;
      x = y;
      y = t;
    }
    const int old = cc_min(&parent[x], y);
    if (old == x) return;
    x = old;
  }
}

// Pass 2.  Grid-stride over the voxels; only pairs whose two voxels lie in different tiles are united.
template <typename T, int CONN>
__global__ __launch_bounds__(256) void cc_merge_kernel(const T* __restrict__ map, int* parent, int n0, int n1, int n2, int nc) {
  const long total = (long)n0 * n1 * n2;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % n2);
    const long r = e / n2;
    const int b = (int)(r % n1), a = (int)(r / n1);
    const int q = seg_class(map, e, nc);
    if (!q) continue;
#pragma unroll
    for (int da = -1; da <= 0; ++da)
#pragma unroll
      for (int db = -1; db <= 1; ++db)
#pragma unroll
        for (int dc = -1; dc <= 1; ++dc) {
          if (!cc_joined<CONN>(da, db, dc)) continue;
          if (da == 0 && (db > 0 || (db == 0 && dc > 0))) continue;      // the neighbours that come first in raster order
          const int xa = a + da, xb = b + db, xc = c + dc;
          if (xa < 0 || xb < 0 || xb >= n1 || xc < 0 || xc >= n2) continue;
          if (xa / kCcT0 == a / kCcT0 && xb / kCcT1 == b / kCcT1 && xc / kCcT2 == c / kCcT2) continue;      // pass 1 joined them
          const long j = ((long)xa * n1 + xb) * n2 + xc;
          if (seg_class(map, j, nc) != q) continue;
          cc_unite(parent, (int)e, (int)j);
        }
  }
}

// Pass 3.  size: in — the tile counts of pass 1 at the tile roots; out — at every component root the component's voxel count.
// A tile root that is not the component's root reads its own slot, which no one adds to; the adds go to component roots only.
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ parent, int* __restrict__ labels, int* size, long total) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int x = parent[e];
    if (x < 0) {
      labels[e] = 0;
      continue;
    }
    for (int p = parent[x]; p != x; p = parent[x]) x = p;
    labels[e] = x + 1;
    if (x != (int)e) {
      const int s = size[e];
      if (s > 0) atomicAdd(&size[x], s);
    }
  }
}

// Pass 4a.  pkey / pcnt: [gridDim.x][kSegMaxClasses], column c for class c.
template <typename T>
__global__ __launch_bounds__(kCcThreads) void cc_reduce_kernel(const T* __restrict__ map, const int* __restrict__ labels,
                                                               const int* __restrict__ size, unsigned long long* __restrict__ pkey,
                                                               int* __restrict__ pcnt, long total, int nc) {
  __shared__ unsigned long long lk[kSegMaxClasses];
  __shared__ int lc[kSegMaxClasses];
  for (int i = threadIdx.x; i < kSegMaxClasses; i += blockDim.x) {
    lk[i] = 0ull;
    lc[i] = 0;
  }
  __syncthreads();
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    if (labels[e] != (int)e + 1) continue;      // not the first voxel of a component
    const int q = seg_class(map, e, nc);
    atomicAdd(&lc[q], 1);
    cc_lds_max64(&lk[q], ((unsigned long long)(unsigned)size[e] << 32) | (unsigned)(kCcIdxMax - (int)e));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSegMaxClasses; i += blockDim.x) {
    pkey[(long)blockIdx.x * kSegMaxClasses + i] = lk[i];
    pcnt[(long)blockIdx.x * kSegMaxClasses + i] = lc[i];
  }
}

// Pass 4b.  One workgroup, thread c for class c: the partials in index order.  rec (workspace) and counts (the caller's, may be null):
// [nc - 1][kCcRec].
__global__ __launch_bounds__(kCcThreads) void cc_finish_kernel(const unsigned long long* __restrict__ pkey, const int* __restrict__ pcnt,
                                                               int parts, long long* __restrict__ rec, long long* __restrict__ counts,
                                                               int nc) {
  const int c = threadIdx.x;
  if (c < 1 || c >= nc) return;
  unsigned long long key = 0ull;
  long long n = 0;
  for (int i = 0; i < parts; ++i) {
    const unsigned long long k = pkey[(long)i * kSegMaxClasses + c];
    if (k > key) key = k;
    n += pcnt[(long)i * kSegMaxClasses + c];
  }
  const long long big = (long long)(key >> 32);
  const long long lab = key ? (long long)(kCcIdxMax - (int)(key & 0xffffffffull)) + 1 : 0;
  long long* r = rec + (long)(c - 1) * kCcRec;
  r[0] = n;
  r[1] = big;
  r[2] = lab;
  if (counts) {
    long long* o = counts + (long)(c - 1) * kCcRec;
    o[0] = n;
    o[1] = big;
    o[2] = lab;
  }
}

// Pass 5.  out may be the map itself: a thread reads and writes its own voxel only.
template <typename T>
__global__ __launch_bounds__(256) void cc_filter_kernel(const T* map, const int* __restrict__ labels, const int* __restrict__ size,
                                                        const long long* __restrict__ rec, T* out, long total, int nc, int keep_largest,
                                                        long long min_size) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int q = seg_class(map, e, nc);
    T v = (T)0;
    if (q) {
      const int l = labels[e];
      if ((!keep_largest || (long long)l == rec[(long)(q - 1) * kCcRec + 2]) && (long long)size[l - 1] >= min_size) v = (T)q;
    }
    out[e] = v;
  }
}

}  // namespace icl
