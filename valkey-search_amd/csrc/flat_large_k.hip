// flat_large_k.hip -- FLAT search with k > 1024 in ONE pass over the rows, gfx950 (option flat-large-k; FlatIndex::search_large_k).
// The paged path (FlatIndex::search_in_passes) scans the whole table once per 1024 results and query; here a chunk of queries
// costs one dense distance pass, a radix select of every query's k-th key over the distances it wrote, and a compaction of
// what lies at or below that key.  The host orders each hand-back and cuts it at k (flat_large_k_host.hpp) -- or, with option
// flat-large-k-device-sort, the device does: a tile sort and merge passes behind the emit (described where they stand).
//
//   flat_dense_distance_kernel   dist[q][row] for rows [0, count) and the qb queries of the block (grid.y = query groups,
//                                flat_scan_pick_qb's choice): the block's queries sit in LDS, a wave owns 16 rows at a time, one
//                                per quad, and every distance is quad_row_distance over the query's fragments -- the function
//                                and the lane layout of K8 / K8b, so the bits are the single-query path's.  A row tile is
//                                fetched from HBM once per block: the qb - 1 further walks over it come out of the cache.  A
//                                row that cannot be an answer (label kNoLabel, rejected by the bitmap) gets a NaN, and NaN is
//                                the one "not a candidate" class from there on: K3 never lists a NaN distance either
//                                (dist <= thr is false).  The waves stride over the row tiles; nothing at or beyond count is
//                                written.
//   flat_large_k_hist_kernel     one digit of the select: grid (slices of kLargeKSlice entries) x (queries).  The block counts
//   flat_large_k_pick_kernel     the digit of every non-NaN entry whose higher digits equal the prefix chosen so far in LDS
//                                bins and adds the bins that are not empty into hist[q][] with one vector atomicAdd each; one
//                                wave per query then finds the bin that holds the k-th entry, extends the prefix, and clears
//                                the bins for the next digit.  Behind the last digit the state holds T (the key of the k-th
//                                smallest candidate, the largest key when there are fewer than k, 0 when there is none),
//                                n_less, n_eq, n_real, a zeroed emit counter and the overflow flag (n_less + n_eq > cap).
//   flat_large_k_emit_kernel     same grid: every candidate with key <= T goes out as (distance bits, labels[row]); a wave
//                                counts its entries over the whole slice first and takes its slots with ONE vector atomicAdd
//                                on the query's counter.  A flagged query writes nothing.
//
// The key is merge_key of flat_scan.hip: order-preserving u32 of the float, -0 and +0 sharing a key.
// Digits: 11 | 11 | 10 bits from the top.  Three digits instead of four (8 x 4) are three walks over the distances and six
// launches instead of four and eight; 2048 bins are 8 KB of LDS per block -- nineteen blocks' worth in a CU's 160 KB, so the
// bins never bound the occupancy -- and one wave still sums them in 32 loads per lane.  Wider digits (16 x 2) would need
// 256 KB of bins.  Distances of one query crowd into a few bins of the top digit; before the LDS atomics a wave takes out
// the lanes that share the first active lane's bin and adds their number once.
//
// No kernel waits for another block: no grid barrier, no spin loop, every loop bound is an argument or a constant.  Plain
// vector loads and stores, LDS, and vector atomics (LDS and global atomicAdd) only; the sort kernels use no atomics.
#include "device_common.hpp"
#include "flat_large_k_host.hpp"
#include "kernels.hpp"

namespace vk {

namespace {

constexpr uint32_t kLargeKThreads = 256;
constexpr uint32_t kLargeKPerThread = 16;
constexpr uint32_t kLargeKSlice = kLargeKThreads * kLargeKPerThread;   // 4096 entries per block of the histogram / emit launches
constexpr uint32_t kLargeKDistBlocks = 2048;                           // row blocks of the distance launch: eight per CU
constexpr int kLargeKDigits = 3;

// digit d covers key bits [shift, shift + width)
__host__ __device__ __forceinline__ uint32_t digit_shift(int d) { return d == 0 ? 21u : d == 1 ? 10u : 0u; }
__host__ __device__ __forceinline__ uint32_t digit_bins(int d) { return d == 2 ? 1024u : 2048u; }

__device__ __forceinline__ uint32_t large_k_dev_key(float f) {   // merge_key (flat_scan.hip)
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <bool kL2, bool kBf16>
__global__ __launch_bounds__(256) void flat_dense_distance_kernel(FlatLargeKArgs a, uint32_t qb) {
  extern __shared__ float4 qs[];   // [qb][chunks][4] float4 = qb padded queries
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 3;
  const int rq = lane >> 2;
  const uint32_t chunks = a.chunks;
  const uint32_t qbase = blockIdx.y * qb;
  const uint32_t per_q = chunks * 4;
  // queries past the chunk's end replicate its last one (never evaluated)
  for (uint32_t i = threadIdx.x; i < per_q * qb; i += blockDim.x) {
    const uint32_t qi = i / per_q, off = i - qi * per_q;
    const uint32_t q = qbase + qi < a.qc ? qbase + qi : a.qc - 1;
    qs[i] = reinterpret_cast<const float4 *>(a.queries + (size_t)q * a.q_stride_f)[off];
  }
  __syncthreads();
  const uint32_t n_q = a.qc - qbase < qb ? a.qc - qbase : qb;   // block-uniform
  const uint32_t total_waves = gridDim.x * 4;
  const uint32_t n_tiles = (a.count + kRowsPerWave - 1) / kRowsPerWave;
  for (uint32_t tile = blockIdx.x * 4 + wave; tile < n_tiles; tile += total_waves) {
    const uint32_t row = tile * kRowsPerWave + rq;
    const bool valid = row < a.count;
    const uint32_t lrow = valid ? row : a.count - 1;
    const char *__restrict__ base = row_base<kBf16>(a.rows, lrow, a.row_stride_f);
    const uint64_t lab = a.labels[lrow];
    const bool cand = lab != kNoLabel && allow_bit(a.allow_bits, a.allow_nbits, lab);
    for (uint32_t qi = 0; qi < n_q; ++qi) {
      const float d = quad_row_distance<kL2, kBf16>(base, qs + (size_t)qi * per_q, chunks, j);
      if (valid && j == 0) a.dist[(size_t)(qbase + qi) * a.ld + row] = cand ? d : __builtin_nanf("");
    }
  }
}

// the thread's entry u of the block's slice: index, or count and beyond = none
__device__ __forceinline__ size_t slice_index(uint32_t u) {
  return (size_t)blockIdx.x * kLargeKSlice + (size_t)u * kLargeKThreads + threadIdx.x;
}

__global__ __launch_bounds__(256) void flat_large_k_hist_kernel(FlatLargeKArgs a, int digit) {
  __shared__ uint32_t s_bin[kLargeKBins];
  const uint32_t q = blockIdx.y;
  const int lane = threadIdx.x & 63;
  for (uint32_t b = threadIdx.x; b < kLargeKBins; b += kLargeKThreads) s_bin[b] = 0;
  __syncthreads();
  const uint32_t shift = digit_shift(digit), mask = digit_bins(digit) - 1u;
  const uint32_t hi_shift = digit == 0 ? 32u : digit == 1 ? 21u : 10u;   // the bits above the digit: they must equal the prefix's
  const uint32_t prefix = digit == 0 ? 0u : a.state[(size_t)q * kLargeKStateWords];
  const float *__restrict__ dist = a.dist + (size_t)q * a.ld;
#pragma unroll 4
  for (uint32_t u = 0; u < kLargeKPerThread; ++u) {
    const size_t i = slice_index(u);
    bool in = false;
    uint32_t bin = 0;
    if (i < a.count) {
      const float d = dist[i];
      const uint32_t key = large_k_dev_key(d);
      in = d == d && (hi_shift == 32u || (key >> hi_shift) == (prefix >> hi_shift));
      bin = (key >> shift) & mask;
    }
    // the lanes that share the first counted lane's bin are added once (one query's distances crowd into a few top digits)
    const uint64_t live = __ballot(in);
    if (live != 0) {
      const int first = __ffsll((unsigned long long)live) - 1;
      const uint32_t fbin = (uint32_t)__builtin_amdgcn_readlane((int)bin, first);
      const uint64_t same = __ballot(in && bin == fbin);
      if (lane == first) atomicAdd(&s_bin[fbin], (uint32_t)__popcll(same));
      else if (in && bin != fbin) atomicAdd(&s_bin[bin], 1u);
    }
  }
  __syncthreads();
  uint32_t *__restrict__ h = a.hist + (size_t)q * kLargeKBins;
  for (uint32_t b = threadIdx.x; b <= mask; b += kLargeKThreads) {
    const uint32_t c = s_bin[b];
    if (c) atomicAdd(&h[b], c);
  }
}

// inclusive prefix over the wave's 64 lanes
__device__ __forceinline__ uint32_t large_k_wave_sum(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// one wave per query: lane l owns bins [l * per, (l + 1) * per)
__global__ __launch_bounds__(64) void flat_large_k_pick_kernel(FlatLargeKArgs a, int digit) {
  const uint32_t q = blockIdx.x;
  const int lane = threadIdx.x;
  uint32_t *__restrict__ h = a.hist + (size_t)q * kLargeKBins;
  uint32_t *__restrict__ st = a.state + (size_t)q * kLargeKStateWords;
  const uint32_t per = digit_bins(digit) / 64u;
  uint32_t sum = 0;
  for (uint32_t i = 0; i < per; ++i) sum += h[lane * per + i];
  const uint32_t inc = large_k_wave_sum(sum, lane);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
  uint32_t prefix = 0, want = a.k, n_less = 0, n_real = total;
  if (digit != 0) {
    prefix = st[0];
    want = st[1];
    n_less = st[2];
    n_real = st[4];
  }
  if (want > total) want = total;   // (digit 0: fewer candidates than k -> the last of them; later digits: never)
  uint32_t bin = 0, below = 0, in_bin = 0;
  if (total != 0) {   // want >= 1
    const uint64_t reach = __ballot(inc >= want);
    const int owner = __ffsll((unsigned long long)reach) - 1;
    if (lane == owner) {
      uint32_t run = inc - sum;
      for (uint32_t i = 0; i < per; ++i) {
        const uint32_t c = h[lane * per + i];
        if (run + c >= want) { bin = lane * per + i; below = run; in_bin = c; break; }
        run += c;
      }
    }
    bin = (uint32_t)__shfl((int)bin, owner);
    below = (uint32_t)__shfl((int)below, owner);
    in_bin = (uint32_t)__shfl((int)in_bin, owner);
  }
  for (uint32_t i = 0; i < per; ++i) h[lane * per + i] = 0;   // the next digit's (the next chunk's) bins
  if (lane == 0) {
    const bool last = digit == kLargeKDigits - 1;
    n_less += below;
    st[0] = prefix | (bin << digit_shift(digit));
    st[1] = want - below;
    st[2] = n_less;
    st[3] = last ? in_bin : 0u;
    st[4] = n_real;
    st[5] = 0;
    st[6] = last && (uint64_t)n_less + in_bin > a.cap ? 1u : 0u;
    st[7] = 0;
  }
}

__global__ __launch_bounds__(256) void flat_large_k_emit_kernel(FlatLargeKArgs a) {
  const uint32_t q = blockIdx.y;
  const int lane = threadIdx.x & 63;
  uint32_t *__restrict__ st = a.state + (size_t)q * kLargeKStateWords;
  if (st[6] != 0) return;   // too many ties at the k-th key: the paged path answers this query
  const uint32_t T = st[0];
  const float *__restrict__ dist = a.dist + (size_t)q * a.ld;
  uint32_t bits[kLargeKPerThread];
  uint32_t sel = 0, mine = 0;
#pragma unroll
  for (uint32_t u = 0; u < kLargeKPerThread; ++u) {
    const size_t i = slice_index(u);
    bits[u] = 0;
    if (i < a.count) {
      const float d = dist[i];
      bits[u] = __float_as_uint(d);
      if (d == d && large_k_dev_key(d) <= T) { sel |= 1u << u; ++mine; }
    }
  }
  const uint32_t inc = large_k_wave_sum(mine, lane);
  const uint32_t wave_total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
  if (wave_total == 0) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(&st[5], wave_total);
  uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)base) + inc - mine;
  uint32_t *__restrict__ ob = a.out_bits + (size_t)q * a.cap;
  uint64_t *__restrict__ ol = a.out_label + (size_t)q * a.cap;
#pragma unroll
  for (uint32_t u = 0; u < kLargeKPerThread; ++u) {
    if ((sel >> u) & 1u) {
      if (at < a.cap) {   // (always: the query is not flagged, so n_less + n_eq <= cap slots are taken in all)
        ob[at] = bits[u];
        ol[at] = a.labels[slice_index(u)];
      }
      ++at;
    }
  }
}

// ---- the device sort of the hand-back (option flat-large-k-device-sort) ---------------------------------------------------------
// A block's 4096 entries live in LDS as two arrays, distance bits (u32) and labels (u64); entry i sits in slot i + i / 16, so
// the 16 consecutive entries a thread takes into registers start 17 slots apart: a wave's loads of "my e-th entry" fall on
// 64 different words instead of on two banks.  4352 slots x 12 B = 51 KB per block, three blocks per CU.
constexpr uint32_t kSortSlots = kLargeKSlice + kLargeKSlice / kLargeKPerThread;
constexpr uint32_t kSortNoBits = 0x7FFFFFFFu;   // the sentinel's distance bits: key 0xFFFFFFFF, above +inf's 0xFF800000
constexpr uint32_t kSortTileLog2 = 12;
static_assert(kLargeKSortTile == kLargeKSlice && (1u << kSortTileLog2) == kLargeKSlice && kLargeKPerThread == 16,
              "the sort's tile is the slice, 16 entries per thread");

__device__ __forceinline__ uint32_t sort_slot(uint32_t i) { return i + (i >> 4); }
__device__ __forceinline__ bool sort_before(uint32_t ka, uint64_t la, uint32_t kb, uint64_t lb) { return ka < kb || (ka == kb && la < lb); }

// the entries a thread holds: key = large_k_dev_key(bits), kept next to the bits (-0 and +0 share a key, the bits differ)
struct SortRegs {
  uint32_t key[kLargeKPerThread], bits[kLargeKPerThread];
  uint64_t lab[kLargeKPerThread];
};
__device__ __forceinline__ void sort_cx(SortRegs &r, uint32_t i, uint32_t l) {   // i < l, constants once unrolled: the smaller one to i
  const bool sw = sort_before(r.key[l], r.lab[l], r.key[i], r.lab[i]);
  const uint32_t ki = r.key[i], bi = r.bits[i];
  const uint64_t li = r.lab[i];
  r.key[i] = sw ? r.key[l] : ki;
  r.bits[i] = sw ? r.bits[l] : bi;
  r.lab[i] = sw ? r.lab[l] : li;
  r.key[l] = sw ? ki : r.key[l];
  r.bits[l] = sw ? bi : r.bits[l];
  r.lab[l] = sw ? li : r.lab[l];
}
// the bitonic network in its all-ascending form: a run of `size` entries is made of two sorted halves by comparing entry i with
// its mirror image in the run (the flip), then by half-cleaners of strides size / 4 ... 1
template <uint32_t kStride>
__device__ __forceinline__ void sort_regs_clean(SortRegs &r) {   // the half-cleaners of strides kStride ... 1 over the 16 entries
  if constexpr (kStride != 0) {
#pragma unroll
    for (uint32_t e = 0; e < kLargeKPerThread; ++e)
      if ((e & kStride) == 0) sort_cx(r, e, e | kStride);
    sort_regs_clean<kStride / 2>(r);
  }
}
template <uint32_t kSize>
__device__ __forceinline__ void sort_regs_all(SortRegs &r) {   // sorts the 16 entries: runs of 2, 4, 8, 16
  if constexpr (kSize <= kLargeKPerThread) {
#pragma unroll
    for (uint32_t e = 0; e < kLargeKPerThread; ++e)
      if ((e ^ (kSize - 1)) > e) sort_cx(r, e, e ^ (kSize - 1));
    sort_regs_clean<kSize / 4>(r);
    sort_regs_all<kSize * 2>(r);
  }
}
// one compare-exchange between two slots of LDS, i < l: the labels are looked at only when the keys do not settle it
__device__ __forceinline__ void sort_lds_cx(uint32_t *s_bits, uint64_t *s_lab, uint32_t i, uint32_t l) {
  const uint32_t si = sort_slot(i), sl = sort_slot(l);
  const uint32_t bi = s_bits[si], bl = s_bits[sl];
  const uint32_t ki = large_k_dev_key(__uint_as_float(bi)), kl = large_k_dev_key(__uint_as_float(bl));
  if (kl <= ki) {
    const uint64_t li = s_lab[si], ll = s_lab[sl];
    if (kl < ki || ll < li) {
      s_bits[si] = bl;
      s_bits[sl] = bi;
      s_lab[si] = ll;
      s_lab[sl] = li;
    }
  }
}
__device__ __forceinline__ void sort_regs_from_lds(SortRegs &r, const uint32_t *s_bits, const uint64_t *s_lab) {
  const uint32_t base = threadIdx.x * (kLargeKPerThread + 1);   // sort_slot(threadIdx.x * 16)
#pragma unroll
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    r.bits[e] = s_bits[base + e];
    r.key[e] = large_k_dev_key(__uint_as_float(r.bits[e]));
    r.lab[e] = s_lab[base + e];
  }
}
__device__ __forceinline__ void sort_regs_to_lds(const SortRegs &r, uint32_t *s_bits, uint64_t *s_lab) {
  const uint32_t base = threadIdx.x * (kLargeKPerThread + 1);
#pragma unroll
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    s_bits[base + e] = r.bits[e];
    s_lab[base + e] = r.lab[e];
  }
}
// a query's entries as the sort sees them: 0 for a flagged query, never beyond cap
__device__ __forceinline__ uint32_t sort_entries(const uint32_t *__restrict__ st, uint32_t cap) {
  if (st[6] != 0) return 0;
  const uint64_t n = (uint64_t)st[2] + st[3];
  return n < cap ? (uint32_t)n : cap;
}

// Tile sort: grid (tiles of 4096 over cap) x (queries).  The block takes entries [tile * 4096, ...) of its query, coalesced
// (which thread starts with which entry does not matter to a sort), sentinels behind n; every thread sorts its 16 in
// registers; the runs of 32 ... 4096 are then made by the flip and the half-cleaners of strides >= 16 on LDS -- eight
// compare-exchanges per thread and step, a barrier behind each -- and the strides 8 ... 1 in registers again.  The sentinels end
// up behind the entries, so the first n - tile * 4096 slots go back where they came from, coalesced; or, with `dense` (cap is
// within one tile: this is the last launch), the first min(k, n) into the dense hand-back.
__global__ __launch_bounds__(256) void flat_large_k_tile_sort_kernel(FlatLargeKSortArgs a, int dense) {
  __shared__ uint32_t s_bits[kSortSlots];
  __shared__ uint64_t s_lab[kSortSlots];
  const uint32_t q = blockIdx.y;
  const uint32_t n = sort_entries(a.state + (size_t)q * kLargeKStateWords, a.cap);
  const uint64_t tile0 = (uint64_t)blockIdx.x * kLargeKSlice;
  if (tile0 >= n) return;   // (a flagged query, a tile behind the entries)
  const uint32_t m = n - (uint32_t)tile0 < kLargeKSlice ? n - (uint32_t)tile0 : kLargeKSlice;   // entries of this tile
  uint32_t *__restrict__ gb = a.bits + (size_t)q * a.cap + tile0;
  uint64_t *__restrict__ gl = a.label + (size_t)q * a.cap + tile0;
  SortRegs r;
#pragma unroll
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    const uint32_t i = e * kLargeKThreads + threadIdx.x;
    r.bits[e] = i < m ? gb[i] : kSortNoBits;
    r.lab[e] = i < m ? gl[i] : kNoLabel;
    r.key[e] = large_k_dev_key(__uint_as_float(r.bits[e]));
  }
  sort_regs_all<2>(r);
  sort_regs_to_lds(r, s_bits, s_lab);
  __syncthreads();
  for (uint32_t size = 2 * kLargeKPerThread; size <= kLargeKSlice; size <<= 1) {
    const uint32_t half = size >> 1;
#pragma unroll 2
    for (uint32_t u = 0; u < kLargeKPerThread / 2; ++u) {   // the flip: entry r of a run's lower half against entry size - 1 - r of the run
      const uint32_t p = u * kLargeKThreads + threadIdx.x, in = p & (half - 1), run0 = (p - in) << 1;
      sort_lds_cx(s_bits, s_lab, run0 + in, run0 + size - 1 - in);
    }
    __syncthreads();
    for (uint32_t stride = size >> 2; stride >= kLargeKPerThread; stride >>= 1) {
#pragma unroll 2
      for (uint32_t u = 0; u < kLargeKPerThread / 2; ++u) {
        const uint32_t p = u * kLargeKThreads + threadIdx.x, in = p & (stride - 1), i = ((p - in) << 1) | in;
        sort_lds_cx(s_bits, s_lab, i, i + stride);
      }
      __syncthreads();
    }
    sort_regs_from_lds(r, s_bits, s_lab);
    sort_regs_clean<kLargeKPerThread / 2>(r);
    sort_regs_to_lds(r, s_bits, s_lab);
    __syncthreads();
  }
  const uint32_t lim = dense ? (a.k < m ? a.k : m) : m;
  uint32_t *__restrict__ ob = dense ? a.dense_bits + (size_t)q * a.k : gb;
  uint64_t *__restrict__ ol = dense ? a.dense_label + (size_t)q * a.k : gl;
#pragma unroll 4
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    const uint32_t i = e * kLargeKThreads + threadIdx.x;
    if (i < lim) {
      ob[i] = s_bits[sort_slot(i)];
      ol[i] = s_lab[sort_slot(i)];
    }
  }
}

// Merge path: of the first o entries of the merge of two sorted runs A (la entries) and B (lb), how many come from A -- an
// entry of A going before an entry of B unless B's is smaller.  at_a / at_b give (key, label) of an entry.  At most 32 steps.
template <class FA, class FB>
__device__ __forceinline__ uint32_t sort_co_rank(uint32_t o, uint32_t la, uint32_t lb, FA at_a, FB at_b) {
  uint32_t lo = o > lb ? o - lb : 0, hi = o < la ? o : la;
  for (int step = 0; step < 32 && lo < hi; ++step) {
    const uint32_t mid = lo + ((hi - lo) >> 1);   // lo <= mid < hi <= la, and 0 <= o - mid - 1 < lb
    uint32_t ka, kb;
    uint64_t xa, xb;
    at_a(mid, ka, xa);
    at_b(o - mid - 1, kb, xb);
    if (sort_before(kb, xb, ka, xa)) hi = mid;   // B's entry is taken before A[mid]: A gives at most mid
    else lo = mid + 1;
  }
  return lo;
}

// Merge pass: grid as the tile sort's.  The sorted runs of run = 4096 << pass entries of src are merged in neighbouring pairs
// into dst; block b owns outputs [b * 4096, (b + 1) * 4096) of its query.  Two threads find the ends of that range in the
// pair's two runs by the merge path over HBM, the block brings the at most 4096 inputs into LDS (A's part in front, B's behind
// it), every thread finds its own 16 outputs' start the same way in LDS and merges them serially into registers; they go
// through LDS once more to leave coalesced.  A run without a partner is the same with an empty B: a copy.  With `last` (one
// pair spans cap) the outputs below min(k, n) go to the dense hand-back and the blocks behind them leave.
__global__ __launch_bounds__(256) void flat_large_k_merge_kernel(FlatLargeKSortArgs a, const uint32_t *__restrict__ src_bits,
                                                                 const uint64_t *__restrict__ src_lab, uint32_t *__restrict__ dst_bits,
                                                                 uint64_t *__restrict__ dst_lab, uint32_t run_log2, int last) {
  __shared__ uint32_t s_bits[kSortSlots];
  __shared__ uint64_t s_lab[kSortSlots];
  __shared__ uint32_t s_cut[2];
  const uint32_t q = blockIdx.y;
  const uint32_t n = sort_entries(a.state + (size_t)q * kLargeKStateWords, a.cap);
  const uint32_t lim = last && a.k < n ? a.k : n;   // outputs anybody wants
  const uint64_t out0 = (uint64_t)blockIdx.x * kLargeKSlice;
  if (out0 >= lim) return;
  const uint64_t pair0 = (out0 >> (run_log2 + 1)) << (run_log2 + 1);   // where this block's pair of runs starts
  const uint64_t run = (uint64_t)1 << run_log2;
  const uint32_t la = (uint32_t)(pair0 + run < n ? run : n - pair0);
  const uint32_t lb = (uint32_t)(pair0 + run >= n ? 0 : (pair0 + 2 * run < n ? run : n - pair0 - run));
  const uint32_t o0 = (uint32_t)(out0 - pair0);
  const uint32_t o1 = (uint64_t)o0 + kLargeKSlice < (uint64_t)la + lb ? o0 + kLargeKSlice : la + lb;   // o0 < la + lb: out0 < n
  const uint32_t *__restrict__ ab = src_bits + (size_t)q * a.cap + pair0;
  const uint64_t *__restrict__ al = src_lab + (size_t)q * a.cap + pair0;
  auto g_a = [&](uint32_t i, uint32_t &key, uint64_t &lab) { key = large_k_dev_key(__uint_as_float(ab[i])); lab = al[i]; };
  auto g_b = [&](uint32_t i, uint32_t &key, uint64_t &lab) { key = large_k_dev_key(__uint_as_float(ab[la + i])); lab = al[la + i]; };
  if (threadIdx.x == 0) s_cut[0] = sort_co_rank(o0, la, lb, g_a, g_b);
  if (threadIdx.x == 64) s_cut[1] = sort_co_rank(o1, la, lb, g_a, g_b);
  __syncthreads();
  // (the cuts of sorted runs are in order and tot apart at most; the clamps keep every index in range whatever the runs hold)
  const uint32_t a0 = s_cut[0], b0 = o0 - a0, tot = o1 - o0;
  const uint32_t na = s_cut[1] < a0 ? 0 : (s_cut[1] - a0 < tot ? s_cut[1] - a0 : tot), nb = tot - na;
#pragma unroll 4
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    const uint32_t i = e * kLargeKThreads + threadIdx.x;
    if (i < tot) {
      uint32_t g = i < na ? a0 + i : la + b0 + (i - na);
      g = g < la + lb ? g : la + lb - 1;
      s_bits[sort_slot(i)] = ab[g];
      s_lab[sort_slot(i)] = al[g];
    }
  }
  __syncthreads();
  auto at = [&](uint32_t i, uint32_t &key, uint64_t &lab) { key = large_k_dev_key(__uint_as_float(s_bits[sort_slot(i)])); lab = s_lab[sort_slot(i)]; };
  auto s_a = [&](uint32_t i, uint32_t &key, uint64_t &lab) { at(i, key, lab); };
  auto s_b = [&](uint32_t i, uint32_t &key, uint64_t &lab) { at(na + i, key, lab); };
  const uint32_t mine0 = threadIdx.x * kLargeKPerThread < tot ? threadIdx.x * kLargeKPerThread : tot;
  const uint32_t mine = tot - mine0 < kLargeKPerThread ? tot - mine0 : kLargeKPerThread;
  uint32_t ia = sort_co_rank(mine0, na, nb, s_a, s_b), ib = mine0 - ia;
  // the two heads; a side that has run out shows the sentinel, which no entry reaches
  uint32_t ka = 0xFFFFFFFFu, kb = 0xFFFFFFFFu, ba = kSortNoBits, bb = kSortNoBits;
  uint64_t xa = kNoLabel, xb = kNoLabel;
  if (ia < na) { ba = s_bits[sort_slot(ia)]; at(ia, ka, xa); }
  if (ib < nb) { bb = s_bits[sort_slot(na + ib)]; at(na + ib, kb, xb); }
  uint32_t out_bits[kLargeKPerThread];
  uint64_t out_lab[kLargeKPerThread];
#pragma unroll
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    const bool from_b = sort_before(kb, xb, ka, xa);
    out_bits[e] = from_b ? bb : ba;
    out_lab[e] = from_b ? xb : xa;
    if (from_b) {
      ++ib;
      kb = 0xFFFFFFFFu, bb = kSortNoBits, xb = kNoLabel;
      if (ib < nb) { bb = s_bits[sort_slot(na + ib)]; at(na + ib, kb, xb); }
    } else {
      ++ia;
      ka = 0xFFFFFFFFu, ba = kSortNoBits, xa = kNoLabel;
      if (ia < na) { ba = s_bits[sort_slot(ia)]; at(ia, ka, xa); }
    }
  }
  __syncthreads();   // every thread has read its inputs: the slots take the outputs
  const uint32_t base = threadIdx.x * (kLargeKPerThread + 1);
#pragma unroll
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    if (e < mine) {
      s_bits[base + e] = out_bits[e];
      s_lab[base + e] = out_lab[e];
    }
  }
  __syncthreads();
  uint32_t *__restrict__ ob = last ? a.dense_bits + (size_t)q * a.k : dst_bits + (size_t)q * a.cap;
  uint64_t *__restrict__ ol = last ? a.dense_label + (size_t)q * a.k : dst_lab + (size_t)q * a.cap;
#pragma unroll 4
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    const uint32_t i = e * kLargeKThreads + threadIdx.x;
    const uint64_t g = out0 + i;
    if (i < tot && g < lim) {
      ob[g] = s_bits[sort_slot(i)];
      ol[g] = s_lab[sort_slot(i)];
    }
  }
}

bool large_k_args_ok(const FlatLargeKArgs &a) {
  return a.count != 0 && a.qc != 0 && a.qc <= kLargeKMaxChunkQueries && a.k != 0 && a.ld >= a.count && a.dist && a.state;
}

}  // namespace

uint32_t flat_large_k_slice() { return kLargeKSlice; }
uint32_t flat_large_k_dist_blocks() { return kLargeKDistBlocks; }

hipError_t launch_flat_large_k_distance(const FlatLargeKArgs &a, bool l2, bool bf16, int qb, hipStream_t s) {
  if (!large_k_args_ok(a) || !a.rows || !a.labels || !a.queries || a.chunks == 0 || a.chunks * 16 != a.row_stride_f || a.q_stride_f < a.row_stride_f ||
      (qb != 1 && qb != 2 && qb != 4 && qb != 8))
    return hipErrorInvalidValue;
  const size_t lds = (size_t)qb * a.chunks * 64;
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  const void *f = l2 ? (bf16 ? reinterpret_cast<const void *>(&flat_dense_distance_kernel<true, true>)
                             : reinterpret_cast<const void *>(&flat_dense_distance_kernel<true, false>))
                     : (bf16 ? reinterpret_cast<const void *>(&flat_dense_distance_kernel<false, true>)
                             : reinterpret_cast<const void *>(&flat_dense_distance_kernel<false, false>));
  if (lds > 48 * 1024) {
    hipError_t e = ensure_max_lds(f);
    if (e != hipSuccess) return e;
  }
  const uint32_t tiles = (a.count + kRowsPerWave - 1) / kRowsPerWave;
  const uint32_t nqg = (a.qc + (uint32_t)qb - 1) / (uint32_t)qb;
  uint32_t blocks = (tiles + 3) / 4;
  if (blocks > kLargeKDistBlocks) blocks = kLargeKDistBlocks;
  FlatLargeKArgs args = a;
  uint32_t qb_arg = (uint32_t)qb;
  void *params[] = {&args, &qb_arg};
  return hipLaunchKernel(f, dim3(blocks, nqg), dim3(256), params, lds, s);
}

hipError_t launch_flat_large_k_select(const FlatLargeKArgs &a, hipStream_t s) {
  if (!large_k_args_ok(a) || !a.hist) return hipErrorInvalidValue;
  const uint32_t slices = (uint32_t)(((uint64_t)a.count + kLargeKSlice - 1) / kLargeKSlice);
  for (int d = 0; d < kLargeKDigits; ++d) {
    hipLaunchKernelGGL(flat_large_k_hist_kernel, dim3(slices, a.qc), dim3(kLargeKThreads), 0, s, a, d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(flat_large_k_pick_kernel, dim3(a.qc), dim3(64), 0, s, a, d);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_flat_large_k_emit(const FlatLargeKArgs &a, hipStream_t s) {
  if (!large_k_args_ok(a) || !a.labels || !a.out_bits || !a.out_label || a.cap == 0) return hipErrorInvalidValue;
  const uint32_t slices = (uint32_t)(((uint64_t)a.count + kLargeKSlice - 1) / kLargeKSlice);
  hipLaunchKernelGGL(flat_large_k_emit_kernel, dim3(slices, a.qc), dim3(kLargeKThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_flat_large_k_sort(const FlatLargeKSortArgs &a, hipStream_t s) {
  if (!a.state || !a.bits || !a.label || !a.dense_bits || !a.dense_label || a.cap == 0 || a.k == 0 || a.qc == 0 || a.qc > kLargeKMaxChunkQueries)
    return hipErrorInvalidValue;
  const uint32_t passes = large_k_sort_passes(a.cap);
  if (passes != 0 && (!a.bits2 || !a.label2)) return hipErrorInvalidValue;
  const uint32_t tiles = (uint32_t)(((uint64_t)a.cap + kLargeKSlice - 1) / kLargeKSlice);
  hipLaunchKernelGGL(flat_large_k_tile_sort_kernel, dim3(tiles, a.qc), dim3(kLargeKThreads), 0, s, a, passes == 0 ? 1 : 0);
  hipError_t e = hipGetLastError();
  for (uint32_t p = 0; p < passes && e == hipSuccess; ++p) {
    const bool odd = (p & 1u) != 0, last = p + 1 == passes;
    // the last pass writes the dense hand-back only: no block beyond min(k, cap) outputs has anything to do
    const uint32_t blocks = last && a.k < a.cap ? (uint32_t)(((uint64_t)a.k + kLargeKSlice - 1) / kLargeKSlice) : tiles;
    hipLaunchKernelGGL(flat_large_k_merge_kernel, dim3(blocks, a.qc), dim3(kLargeKThreads), 0, s, a, odd ? a.bits2 : a.bits,
                       odd ? a.label2 : a.label, odd ? a.bits : a.bits2, odd ? a.label : a.label2, kSortTileLog2 + p, last ? 1 : 0);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace vk
