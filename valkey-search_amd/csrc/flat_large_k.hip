// flat_large_k.hip -- FLAT search with k > 1024 in ONE pass over the rows, gfx950 (option flat-large-k; FlatIndex::search_large_k).
// The paged path (FlatIndex::search_in_passes) scans the whole table once per 1024 results and query; here a chunk of queries
// costs one dense distance pass, a radix select of every query's k-th key over the distances it wrote, and a compaction of
// what lies at or below that key.  The host orders each hand-back and cuts it at k (flat_large_k_host.hpp).
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
// vector loads and stores, LDS, and vector atomics (LDS and global atomicAdd) only.
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

}  // namespace vk
