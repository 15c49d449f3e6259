// rankindex.h — where to crop: the centre draws of MONAI's RandCropByPosNegLabeld (utils/data_utils.py:84-99 of the reference,
// get_loader) without an index list per voxel.  MONAI keeps flatnonzero(label != 0) and flatnonzero((image > t) & (label == 0)) per
// cached volume on the host, 8 B a voxel; the host then draws "the r-th foreground voxel".  Here the volume stays in HBM and a RANK
// INDEX answers the same question: the flattened (C-order) volume is cut into tiles of kRankTile consecutive voxels, and per list one
// uint32 array of tiles + 1 entries holds the exclusive prefix of the tiles' member counts (entry t: members before tile t; the last
// entry: the list's length) — 8 B per 1,024 voxels.
//   members:  fg = label != 0;  bg = label == 0 && image > threshold (a NaN voxel is not > t)
//   build, once per volume:  rank_count_kernel (one workgroup per tile: members counted per thread, summed per wave with shuffles and
//       over the four waves in index order) -> rank_scan_kernel (one workgroup per list walks the counts in chunks of 1,024 with a
//       carried total).  Integers only, no atomics: the index is a function of the volume alone.
//   select, per sample:  rank_select_kernel (one workgroup per sample): binary search of the prefix for the tile that holds rank r
//       (every lane runs the same search on the same addresses), the tile's 1,024 voxels are loaded once, the per-thread member counts
//       go through a workgroup exclusive scan, the thread whose range holds r - prefix[tile] finds the voxel; thread 0 unravels it,
//       applies correct_crop_centers + SpatialCrop (origin = clamp(centre - s / 2, 0, n - s)) and stores the three int32.
#pragma once

namespace icl {

constexpr int kRankTile = 1024;                              // consecutive flat voxels per index entry
constexpr int kRankThreads = 256;
constexpr int kRankPer = kRankTile / kRankThreads;           // consecutive voxels (or index entries, in the scan) per thread
constexpr int kRankFg = 0, kRankBg = 1;                      // which list a sample is drawn from
static_assert(kRankPer == 4, "one float4 of image and one dword of labels per thread");

// The thread's kRankPer voxels from flat index `first` on: bit t = voxel first + t is foreground, bit 4 + t = it is background
// above the threshold.  Voxels at or past `total` are members of nothing.  vec: image 16-byte and label 4-byte aligned (first is a
// multiple of 4), so a whole group is one 16-byte and one 4-byte load.
__device__ __forceinline__ unsigned rank_members(const float* __restrict__ image, const uint8_t* __restrict__ label, long first, long total,
                                                 float thr, bool vec) {
  float x[kRankPer];
  unsigned lab[kRankPer];
  bool in[kRankPer];
  if (vec && first + kRankPer <= total) {
    const float4 v = *reinterpret_cast<const float4*>(image + first);
    const unsigned l = *reinterpret_cast<const unsigned*>(label + first);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
#pragma unroll
    for (int t = 0; t < kRankPer; ++t) {
      lab[t] = (l >> (8 * t)) & 255u;
      in[t] = true;
    }
  } else {
#pragma unroll
    for (int t = 0; t < kRankPer; ++t) {
      in[t] = first + t < total;
      x[t] = in[t] ? image[first + t] : 0.f;
      lab[t] = in[t] ? (unsigned)label[first + t] : 0u;
    }
  }
  unsigned m = 0;
#pragma unroll
  for (int t = 0; t < kRankPer; ++t) {
    if (in[t] && lab[t] != 0u) m |= 1u << t;
    if (in[t] && lab[t] == 0u && x[t] > thr) m |= 16u << t;      // NaN > thr is false
  }
  return m;
}

// clamp(v, 0, hi)
__device__ __forceinline__ int rank_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned rank_pop4(unsigned m) { return (m & 1u) + ((m >> 1) & 1u) + ((m >> 2) & 1u) + ((m >> 3) & 1u); }

// inclusive prefix sum over the 64 lanes of a wave (every lane of the wave must call it)
__device__ __forceinline__ unsigned rank_wave_scan(unsigned v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl(v, (lane - d) & 63, 64);
    if (lane >= d) v += up;
  }
  return v;
}

// Exclusive prefix of `v` over the workgroup's kRankThreads threads, in thread order.  `wsum`: kRankThreads / 64 words of LDS; the
// caller must not reuse it before its next __syncthreads.  One barrier inside.
__device__ __forceinline__ unsigned rank_block_scan(unsigned v, unsigned* wsum, unsigned& block_total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned inc = rank_wave_scan(v, lane);
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kRankThreads / 64; ++w) {
    if (w < wave) before += wsum[w];
    all += wsum[w];
  }
  block_total = all;
  return before + inc - v;
}

// grid (tiles), kRankThreads threads.  fg[t + 1] / bg[t + 1] = the member counts of tile t (rank_scan_kernel makes prefixes of them).
__global__ __launch_bounds__(kRankThreads) void rank_count_kernel(const float* __restrict__ image, const uint8_t* __restrict__ label,
                                                                  unsigned* __restrict__ fg, unsigned* __restrict__ bg, long total, float thr,
                                                                  int vec) {
  __shared__ unsigned part[2][kRankThreads / 64];
  const long first = (long)blockIdx.x * kRankTile + (long)threadIdx.x * kRankPer;
  const unsigned m = rank_members(image, label, first, total, thr, vec != 0);
  unsigned cf = rank_pop4(m), cb = rank_pop4(m >> 4);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    cf += __shfl_down(cf, d, 64);
    cb += __shfl_down(cb, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = cf;
    part[1][threadIdx.x >> 6] = cb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned sf = 0, sb = 0;
#pragma unroll
    for (int w = 0; w < kRankThreads / 64; ++w) {
      sf += part[0][w];
      sb += part[1][w];
    }
    fg[blockIdx.x + 1] = sf;
    bg[blockIdx.x + 1] = sb;
  }
}

// grid (2): workgroup 0 the foreground array, workgroup 1 the background array; kRankThreads threads.  In place: entries 1..tiles
// hold counts going in and inclusive sums coming out, entry 0 becomes 0 — so entry t is the exclusive prefix of tile t and entry
// `tiles` the total.
__global__ __launch_bounds__(kRankThreads) void rank_scan_kernel(unsigned* __restrict__ fg, unsigned* __restrict__ bg, int tiles) {
  __shared__ unsigned wsum[kRankThreads / 64];
  unsigned* __restrict__ p = blockIdx.x ? bg : fg;
  if (threadIdx.x == 0) p[0] = 0u;
  unsigned carry = 0;
  for (int base = 1; base <= tiles; base += kRankTile) {      // the trip count is the same for every thread: barriers inside
    const int i0 = base + (int)threadIdx.x * kRankPer;
    unsigned v[kRankPer], s = 0;
#pragma unroll
    for (int t = 0; t < kRankPer; ++t) {
      v[t] = i0 + t <= tiles ? p[i0 + t] : 0u;
      s += v[t];
    }
    unsigned chunk;
    unsigned run = carry + rank_block_scan(s, wsum, chunk);
#pragma unroll
    for (int t = 0; t < kRankPer; ++t) {
      run += v[t];
      if (i0 + t <= tiles) p[i0 + t] = run;
    }
    carry += chunk;
    __syncthreads();      // wsum is written again in the next round
  }
}

struct RankSelectSample {
  const float* image;        // [n0][n1][n2] fp32
  const uint8_t* label;      // [n0][n1][n2] uint8
  const unsigned* prefix;    // the chosen list's index: tiles + 1 entries
  int tiles;                 // ceil(n0 n1 n2 / kRankTile)
  int kind;                  // kRankFg / kRankBg
  int rank;                  // 0 <= rank < prefix[tiles] (the host's check: only the host knows the totals)
  int n0, n1, n2;            // extents
  int s0, s1, s2;            // crop size, min(R, n) per axis
  int vec;                   // image 16-byte and label 4-byte aligned
};

struct RankSelectBatch {
  RankSelectSample s[kFeedMaxBatch];     // 72 B a record: 1,152 B of the 4 KB kernel-argument block
};

// grid (B), kRankThreads threads.  origins [B][3] int32.  Every read stays inside the index and the volume whatever the rank: a rank at
// or past the list's length (which the host refuses) selects voxel 0, so an origin is always written and always in [0, n - s].
__global__ __launch_bounds__(kRankThreads) void rank_select_kernel(RankSelectBatch sb, float thr, int* __restrict__ origins) {
  __shared__ unsigned wsum[kRankThreads / 64];
  __shared__ int chosen;
  const RankSelectSample& s = sb.s[blockIdx.x];              // one sample per workgroup: the record and the search are wave-uniform
  const unsigned r = (unsigned)s.rank;
  if (threadIdx.x == 0) chosen = 0;
  int lo = 0, hi = s.tiles;                                   // prefix[lo] <= r throughout; ends at the last tile with prefix <= r
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s.prefix[mid] <= r) lo = mid; else hi = mid;
  }
  const unsigned local = r - s.prefix[lo];
  const long total = (long)s.n0 * s.n1 * s.n2;
  const long first = (long)lo * kRankTile + (long)threadIdx.x * kRankPer;
  unsigned m = rank_members(s.image, s.label, first, total, thr, s.vec != 0);
  if (s.kind == kRankBg) m >>= 4;
  m &= 15u;
  const unsigned cnt = rank_pop4(m);
  unsigned in_tile;
  const unsigned before = rank_block_scan(cnt, wsum, in_tile);      // the barrier inside also orders `chosen = 0` before the write below
  if (local >= before && local < before + cnt) {
    unsigned k = local - before;
    int at = 0;
#pragma unroll
    for (int t = kRankPer - 1; t >= 0; --t)                   // the k-th set bit of m
      if (rank_pop4(m & ((1u << t) - 1u)) == k && (m >> t & 1u)) at = t;
    chosen = (int)(first + at);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int idx = chosen;
    const int i2 = idx % s.n2, rest = idx / s.n2;
    const int i1 = rest % s.n1, i0 = rest / s.n1;
    const int o0 = rank_clamp(i0 - s.s0 / 2, s.n0 - s.s0);
    const int o1 = rank_clamp(i1 - s.s1 / 2, s.n1 - s.s1);
    const int o2 = rank_clamp(i2 - s.s2 / 2, s.n2 - s.s2);
    int* o = origins + 3 * blockIdx.x;
    o[0] = o0;
    o[1] = o1;
    o[2] = o2;
  }
}

}  // namespace icl
