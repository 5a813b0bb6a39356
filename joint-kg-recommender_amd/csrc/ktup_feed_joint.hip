// Device-fed steps of the joint baselines (coFM, CKE, CFKG): the two pieces of host work that stood between a feed launch
// (ktup_feed_rec / ktup_feed_kg, ktup_sample.hip) and their step kernels.
//   ktup_feed_remap_ids   : raw item / entity ids -> rows of the joint table under -share_embeddings
//                           (knowledgable_recommendation.py:326-328, :352-356: `[i_map[i] for i in ...]`, `[e_map[e] for e in ...]`);
//   ktup_feed_align_lists : the alignment lists of coFM with its own item table (:28-37 getMappedEntities, :39-48 getMappedItems):
//                           the DISTINCT ids of the batch that have a partner in the other space, with that partner.
// Both are one launch with static arguments, so they replay inside the step's HIP graph; neither issues a memset, and neither keeps
// scratch in global memory: the dedupe table lives in LDS and is rebuilt by every launch.
#include "ktup_common.h"

using namespace ktup;

namespace {

constexpr int REMAP_THREADS = 256;
constexpr int ALIGN_THREADS = 1024;
constexpr uint32_t EMPTY = 0xffffffffu;                   // no id reaches 2^31 (n_partner < 2^31 is checked on the host)
constexpr int SMALL_LOG2 = 12, LARGE_LOG2 = 15;           // 4096 slots (16 KiB) for <= 2048 ids, 32768 slots (128 KiB) for <= 16384
constexpr int64_t ALIGN_MAX_IDS = (int64_t)1 << (LARGE_LOG2 - 1);

__global__ __launch_bounds__(REMAP_THREADS) void feed_remap_ids_kernel(const int64_t* __restrict__ row_of_id, int64_t n_map, int64_t* a,
                                                                        int64_t na, int64_t* b, int64_t nb,
                                                                        int32_t* __restrict__ fail) {
  for (int64_t k = (int64_t)blockIdx.x * REMAP_THREADS + threadIdx.x; k < na + nb; k += (int64_t)gridDim.x * REMAP_THREADS) {
    int64_t* x = k < na ? a + k : b + (k - na);
    const int64_t id = *x;
    int64_t row = (id >= 0 && id < n_map) ? row_of_id[id] : -1;
    if (row < 0) {                                         // unmapped: an in-range stand-in + the error count, like the samplers
      if (fail) atomicAdd(fail, 1);
      row = 0;
    }
    *x = row;
  }
}

// One workgroup.  tab[]: open addressing with linear probing, keyed by id, at most half full (the host picks LOG2).  The thread
// whose compare-and-swap turns an EMPTY slot into its id is that id's first claimant and emits the pair; a thread that finds its
// own id already there drops out.  Output positions: one LDS add per wave (ballot + prefix count), not one per pair.
template <int LOG2>
__global__ __launch_bounds__(ALIGN_THREADS) void feed_align_lists_kernel(const int64_t* __restrict__ a, int64_t na,
                                                                          const int64_t* __restrict__ b, int64_t nb,
                                                                          const int64_t* __restrict__ partner, int64_t n_partner,
                                                                          int ids_are_entities, int64_t* __restrict__ n_out,
                                                                          int64_t* __restrict__ e_ids, int64_t* __restrict__ i_ids) {
  constexpr uint32_t SLOTS = 1u << LOG2, MASK = SLOTS - 1u;
  __shared__ uint32_t tab[SLOTS];
  __shared__ uint32_t count;
  const int tid = threadIdx.x;
  for (uint32_t s = tid; s < SLOTS; s += ALIGN_THREADS) tab[s] = EMPTY;
  if (tid == 0) count = 0u;
  __syncthreads();
  const int64_t n = na + nb;
  const int64_t n_up = (n + 63) & ~(int64_t)63;            // whole waves take every trip: the ballot below sees all 64 lanes
  for (int64_t k = tid; k < n_up; k += ALIGN_THREADS) {
    int64_t id = -1, other = -1;
    if (k < n) {
      id = k < na ? a[k] : b[k - na];
      if (id >= 0 && id < n_partner) other = partner[id];
    }
    bool first = false;
    if (other >= 0) {
      const uint32_t key = (uint32_t)id;
      uint32_t slot = (key * 2654435761u) >> (32 - LOG2);
      for (;;) {                                           // ends: the table holds at most n <= SLOTS / 2 keys
        const uint32_t old = atomicCAS(&tab[slot], EMPTY, key);
        if (old == EMPTY) { first = true; break; }
        if (old == key) break;
        slot = (slot + 1u) & MASK;
      }
    }
    const unsigned long long votes = __ballot(first);
    if (votes) {
      const int lane = tid & 63;
      const int leader = __ffsll((long long)votes) - 1;
      uint32_t base = 0u;
      if (lane == leader) base = atomicAdd(&count, (uint32_t)__popcll(votes));
      base = __shfl(base, leader, 64);
      if (first) {
        const uint32_t pos = base + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));      // < count <= n <= cap
        e_ids[pos] = ids_are_entities ? id : other;
        i_ids[pos] = ids_are_entities ? other : id;
      }
    }
  }
  __syncthreads();
  if (tid == 0) *n_out = (int64_t)count;
}

}  // namespace

extern "C" int ktup_feed_remap_ids(const int64_t* row_of_id, int64_t n_ids_in_map, int64_t* a, int64_t na, int64_t* b, int64_t nb,
                                   int32_t* fail_count, void* stream) {
  const char* name = "ktup_feed_remap_ids";
  KTUP_REQUIRE(na >= 0 && nb >= 0 && n_ids_in_map > 0, "%s: bad sizes", name);
  KTUP_REQUIRE(row_of_id, "%s: null table", name);
  KTUP_REQUIRE((a || na == 0) && (b || nb == 0), "%s: null id array", name);
  if (na + nb == 0) return KTUP_OK;
  hipLaunchKernelGGL(feed_remap_ids_kernel, dim3(grid_for((na + nb + REMAP_THREADS - 1) / REMAP_THREADS)), dim3(REMAP_THREADS), 0,
                     (hipStream_t)stream, row_of_id, n_ids_in_map, a, na, b, nb, fail_count);
  return check_launch(name);
}

extern "C" int ktup_feed_align_lists_supported(int64_t n_ids) { return n_ids >= 1 && n_ids <= ALIGN_MAX_IDS ? 1 : 0; }

extern "C" size_t ktup_feed_align_lists_workspace_bytes(int64_t n_ids) {
  (void)n_ids;
  return 0;                                                // the table is LDS
}

extern "C" int ktup_feed_align_lists(const int64_t* a, int64_t na, const int64_t* b, int64_t nb, const int64_t* partner,
                                     int64_t n_partner, int ids_are_entities, int64_t cap, int64_t* n_out, int64_t* e_ids,
                                     int64_t* i_ids, void* ws, void* stream) {
  const char* name = "ktup_feed_align_lists";
  KTUP_REQUIRE(na >= 0 && nb >= 0 && na + nb > 0, "%s: no ids (na = %lld, nb = %lld)", name, (long long)na, (long long)nb);
  KTUP_REQUIRE((a || na == 0) && (b || nb == 0), "%s: null id array", name);
  KTUP_REQUIRE(partner && n_out && e_ids && i_ids, "%s: null pointer argument", name);
  KTUP_REQUIRE(n_partner > 0 && n_partner < (1ll << 31), "%s: n_partner %lld outside [1, 2^31)", name, (long long)n_partner);
  KTUP_REQUIRE(cap >= na + nb, "%s: cap %lld < na + nb = %lld", name, (long long)cap, (long long)(na + nb));
  KTUP_REQUIRE(ws || ktup_feed_align_lists_workspace_bytes(na + nb) == 0, "%s: null workspace", name);
  if (!ktup_feed_align_lists_supported(na + nb))
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: %lld ids, at most %lld", name, (long long)(na + nb), (long long)ALIGN_MAX_IDS);
  hipStream_t st = (hipStream_t)stream;
  if (na + nb <= (1ll << (SMALL_LOG2 - 1)))
    hipLaunchKernelGGL(feed_align_lists_kernel<SMALL_LOG2>, dim3(1), dim3(ALIGN_THREADS), 0, st, a, na, b, nb, partner, n_partner,
                       ids_are_entities, n_out, e_ids, i_ids);
  else
    hipLaunchKernelGGL(feed_align_lists_kernel<LARGE_LOG2>, dim3(1), dim3(ALIGN_THREADS), 0, st, a, na, b, nb, partner, n_partner,
                       ids_are_entities, n_out, e_ids, i_ids);
  return check_launch(name);
}
