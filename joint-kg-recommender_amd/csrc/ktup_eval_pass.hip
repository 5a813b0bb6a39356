// K16 + K17 fused for a whole evaluation pass (soft gate, squared L2): all-item TUP / KTUP scores AND the filtered top-n of
// every user in ONE sweep that never writes the (users x items) score matrix.
//
// Reference: transUP.py:84-102 / jTransUP.py:163-191 (evaluate / evaluateRec) produce a (B x N) matrix per batch of 512 users,
// which utils/misc.py:186-248 copies to the host, argsorts and walks.  Round 1 kept that shape on the device: per batch a
// six-GEMM score kernel wrote B x N x 4 bytes (78 MB over an ml1m pass) and a ranking kernel read them back -- 12 batches x
// ~5 launches, 1.05 ms.  Here:
//   * scores: |a|^2 - 2 s (a.n) + s^2 |n|^2 as in pairs_l2_mc_kernel (ktup_eval_mc.hip), but with every user x item cross term
//     except u.v contracted in PREFERENCE space (see QGeom below): 68 instead of 156 MFMAs per 16 x 16 tile at d = 100, P = 20.
//     Scores agree with the matrix route to fp32 rounding (the same sums in another association);
//   * a workgroup owns 64 users (4 waves x 16) and a contiguous split of the catalogue.  A wave keeps its 16 users' operand
//     rows in REGISTERS for the whole pass (17 float4 per lane); items stream through a double-buffered LDS buffer of
//     16-item tiles (the B operands, 160 floats per item) that the next tile's global loads refill under the MFMAs -- three
//     workgroups per CU;
//   * ranking: a user's sorted top-n list (64-bit keys = order-preserving score image << 32 | item id, the order of
//     ktup_rank.hip: ascending score, ties -> lower id) lives in the wave's LDS and is touched only when 16 candidates are pending
//     for it.  A score is a candidate if it is below the user's n-th score -- compared as floats, the keys deciding equality --
//     and its bit in the wave's filter bitmap (built once from the CSR filter lists, for this workgroup's item split only: 16 users
//     x (split / 32) words of LDS) is clear; candidates go to the user's pending row at positions taken from a ballot, and a row
//     that holds 16 is merged with the list by a fixed 16-lane network (bitonic sort of the candidates + merge: DPP exchanges on
//     the four rows of a register slot at once).  (History: lists in LDS with one insertion per wave at a time: 830 us per ml1m
//     pass; lists in registers with the network run per tile and slot: 212 us, 400 of its ~670 VALU instructions per tile in the
//     network; deferred merges: ~380 per tile, 192 us.  What is left is the shared MFMA + VALU pipe at the clock the chip holds
//     under this load (~2.1 GHz): option dbg_eval switches phases off to measure them -- 120 us without the ranking, 23 us of
//     prologue per workgroup.);
//   * both operand tables and the per-row scalars are built per pass by one small launch (pspace_rows_kernel) after the three
//     P x P Gram matrices (pspace_gram_kernel); the splits' partial lists are merged by a last, tiny launch (topk_merge_kernel).
//   * cut-offs above 16 (ktup_eval_pref_topk_wide): the list is SEG = 2 (topn <= 32) or 4 (topn <= 64) of ktup_topn.h's 16-key
//     segments, [16][SEG][16] keys per wave, merged by row_merge_pending_wide; everything that makes a score, the candidate test, the
//     filter bit and the append are the same code, so a (user, item) score is the same bits on either entry point.  A segment adds
//     2 KB per wave: two workgroups per CU instead of three, at most 512 / topn splits (and 8), the merge over up to 512 keys per user
//     (topk_merge_kernel<8, .>).  SEG = 1 is the narrow entry point's kernel, the machine code it was before the parameter existed;
//   * d = 256 (QGeom<64, NP>): 71 / 99 / 120 operand registers a lane at P <= 4 / 20 / 32 (188 / 222 / 244 VGPRs in all, no scratch: two
//     workgroups per CU, as at d = 128 with P > 4), tiles of 17.7 / 20.7 / 22.8 KB; the operand rows of P > 4 come from pspace_rows_kernel
//     (RGeom<64, 5 | 8>::LDS is 176 / 182 KB: launch_q's ROWS_MC_FITS).  The callers take this width by option eval_q256;
// L1 distance and the ST-Gumbel gate do not decompose into bilinear terms: the hard gate has its own sweep (ktup_eval.hip
// sweep_hard_kernel, either distance); the soft gate with L1 keeps the per-batch kernels of ktup_eval.hip.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ktup_common.h"
#include "ktup_lane_swap.h"
#include "ktup_pref_geom.h"
#include "ktup_pref_q_tile.h"
#include "ktup_topn.h"

namespace ktup {
namespace {

// LDS per wave of the sweep: user scalars [16][4] | filter bits [16][bm_words] | pending candidates [16][PCAP] u64 | lists [16][SEG][16]
// u64 | n-th keys [16] u64.  SEG: 16-key segments of a user's list (ktup_topn.h: 1 = the narrow list, 2 or 4 = the wide ones).  The
// kernel finds the last three from the END of its wave's share: WAVE_TAIL<SEG> is the one place that says how long that end is, for the
// kernel and for the launch's LDS size alike.
template <int SEG>
constexpr size_t WAVE_TAIL = (size_t)16 * PCAP * 8 + (size_t)16 * 16 * SEG * 8 + (size_t)16 * 8;
template <int SEG>
constexpr size_t wave_lds_bytes(int bm_words) { return (((size_t)16 * 4 * 4 + (size_t)16 * bm_words * 4 + 7) & ~(size_t)7) + WAVE_TAIL<SEG>; }
// Workgroups per CU the sweep is bounded and split for.  Narrow: what the registers allow (QGeom::MINW; ~50 KB of LDS at d = 100,
// P = 20 and ml1m-size splits: three fit).  Wide: a segment adds 2 KB per wave, 8 KB per workgroup -- ~58 KB with two, ~74 KB with
// four: two workgroups per CU, and 256 registers a lane.
template <typename G, int SEG>
constexpr int q_wgs() { return SEG == 1 ? G::MINW : 2; }

// The filter lists of a pass as bits, built ONCE per pass instead of once per catalogue split inside the sweep (where the walk was 15 of
// the sweep's 180 us: every split's workgroup of a user block repeated it, latency-bound, before its first tile): one wave per 16
// consecutive users walks their contiguous run of the CSR ids -- all 64 lanes together, sixteen loads in flight per lane, an entry's
// row found by comparing its position with the 15 inner offsets --, sets bit (id - split's first item) of word [row][split][.] in
// LDS and stores the 16 rows as one contiguous run: out[(user * nsplit + split) * bm_words + word].  The waves ride as extra
// workgroups of the Gram launch (which the sweep waits for anyway).
struct FiltBm {
  const int64_t* off; const int32_t* ids; int64_t nq, n_items; uint32_t* out; int nsplit, bm_words; uint32_t split_items; int gram_blocks;
};

KTUP_DEV void filter_bitmap_wave(const FiltBm& f, int64_t u0, uint32_t* lbm, int lane) {
  const int wpu = f.nsplit * f.bm_words;
  for (int idx = lane; idx < 16 * wpu; idx += 64) lbm[idx] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int64_t uo = u0 + (lane < 16 ? lane : 16);
  const int64_t myoff = f.off[uo < f.nq ? uo : f.nq];
  const int64_t f_begin = __shfl(myoff, 0, 64), f_end = __shfl(myoff, 16, 64);
  uint32_t rel[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) rel[k] = (uint32_t)(__shfl(myoff, k + 1, 64) - f_begin);
  constexpr int FB = 16;                                               // loads in flight per lane
  for (int64_t base = f_begin; base < f_end; base += 64 * FB) {
    int32_t ids[FB];
#pragma unroll
    for (int k = 0; k < FB; ++k) {
      const int64_t e = base + lane + 64 * k;
      ids[k] = e < f_end ? f.ids[e] : -1;
    }
#pragma unroll
    for (int k = 0; k < FB; ++k) {
      const uint32_t pos = (uint32_t)(base - f_begin) + lane + 64 * k;
      int r = 0;
#pragma unroll
      for (int q = 0; q < 15; ++q) r += pos >= rel[q] ? 1 : 0;
      if (ids[k] >= 0 && ids[k] < f.n_items) {
        const uint32_t id = (uint32_t)ids[k], sp = id / f.split_items, lid = id - sp * f.split_items;
        atomicOr(lbm + r * wpu + sp * f.bm_words + (lid >> 5), 1u << (lid & 31));
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  uint32_t* o = f.out + u0 * wpu;                                      // (sized for whole 64-user blocks: rows past nq are all-zero)
  for (int idx = lane; idx < 16 * wpu; idx += 64) o[idx] = lbm[idx];
}

// ================================================================================================ preference-space formulation
// QGeom, the A-operand load, the tile DMA, the MFMA chain and the score formula: ktup_pref_q_tile.h (shared with the rank pass,
// ktup_pref_rank_pass.hip)

struct QArgs {
  const float *A, *SCU;          // users: AROW floats + 4 scalars each
  const float* B;                // items: rows of GROW floats (operands, then the 4 scalars)
  int64_t nq, n_items;
  const int64_t* filt_off; const int32_t* filt_ids;
  int topn, nsplit; int64_t split_items; uint64_t* part; int bm_words;
  int32_t* gthr;                 // [nq (+ pad to whole 64-user blocks)] the best n-th score any split of a user has reached, as the bits of a
                                 // non-negative float (0x7fffffff: none yet); see the tile loop
  const uint32_t* bmg;           // the filter lists as bits, [user][split][bm_words] (filter_bitmap_wave); NULL: the sweep walks the lists itself
  int dbg;                       // MEASUREMENT ONLY (option dbg_eval): 1 no ranking epilogue, 2 no item loads, 4 no workgroup barrier per tile, 8 no tiles at all
};

template <typename G, int SEG = 1>
__global__ __launch_bounds__(256, (q_wgs<G, SEG>())) void eval_pass_q_kernel(QArgs a) {
  static_assert(SEG == 1 || SEG == 2 || SEG == 4, "a list is one, two or four 16-key segments");
  constexpr int RB4 = G::RB4, ROW4 = G::ROW4;
  static_assert(G::SUB == 1, "one 16-item tile per buffer");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4* Xb = reinterpret_cast<v4*>(smem);                                   // [2][TILE_F4] item tiles
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* wbase = reinterpret_cast<char*>(Xb + 2 * G::TILE_F4) + (size_t)w * wave_lds_bytes<SEG>(a.bm_words);
  float* usc = reinterpret_cast<float*>(wbase);                           // [16][4] user scalars
  uint32_t* bm = reinterpret_cast<uint32_t*>(usc + 64);                   // [16][bm_words] filter bits of this split
  uint64_t* pbuf = reinterpret_cast<uint64_t*>(wbase + wave_lds_bytes<SEG>(a.bm_words) - WAVE_TAIL<SEG>);   // [16][PCAP] pending candidates
  uint64_t* tk = pbuf + 16 * PCAP;                                        // [16][SEG][16] the users' sorted lists (touched by merges only)
  uint64_t* thrk = tk + 16 * 16 * SEG;                                         // [16] their n-th keys (read where floats cannot decide)
  // Which (user block, split) this workgroup takes: workgroups go to the 8 XCDs round-robin in launch order and every XCD has an L2 of
  // its own, so with (blockIdx.x, blockIdx.y) taken as they come the 8 splits of a user block sit on 8 different XCDs and EVERY L2
  // fetches EVERY user row (8 x 6.6 MB over the fabric at ml1m size, ~10 us of prologue).  XCD x (launch-order ids x, x + 8, ...) takes
  // a contiguous run of the pairs ordered user block major instead: its L2 then holds ~1/8 of the user rows (the item rows it needs
  // entirely either way).
  int ub, sp;
  {
    const uint32_t L = blockIdx.x + gridDim.x * blockIdx.y, total = gridDim.x * gridDim.y;
    const uint32_t x = L & 7u, per = total >> 3, rem = total & 7u;
    const uint32_t q = x * per + (x < rem ? x : rem) + (L >> 3);
    ub = (int)(q / (uint32_t)a.nsplit);
    sp = (int)(q - (uint32_t)ub * (uint32_t)a.nsplit);
  }
  const int64_t u0 = (int64_t)ub * 64 + 16 * w;
  const int64_t i_lo = (int64_t)sp * a.split_items;
  const int64_t i_hi = min(a.n_items, i_lo + a.split_items);
  const int topn = a.topn;
  // the wave's filter bits from the pass's bitmap (filter_bitmap_wave): requested first, stored after the other set-up work below
  constexpr int BMR = 8;                                                  // words per lane held in flight (more: a second trip)
  const bool use_bmg = a.bmg != nullptr && a.filt_off && !(a.dbg & 16);
  uint32_t bmv[BMR];
  if (use_bmg) {
    const int nw = 16 * a.bm_words;
#pragma unroll
    for (int k = 0; k < BMR; ++k) {
      const int idx = lane + 64 * k, r = idx / a.bm_words;
      bmv[k] = idx < nw ? a.bmg[((u0 + r) * a.nsplit + sp) * a.bm_words + (idx - r * a.bm_words)] : 0u;
    }
  }
  for (int idx = tid; idx < 2 * G::TILE_F4; idx += 256) Xb[idx] = (v4){0.f, 0.f, 0.f, 0.f};   // row pads stay finite (x 0 operands)
  if (!use_bmg)
    for (int idx = lane; idx < 16 * a.bm_words; idx += 64) bm[idx] = 0u;
  for (int idx = lane; idx < 16 * 16 * SEG; idx += 64) tk[idx] = PKEY_MAX;   // every segment of every list
  if (lane < 16) thrk[lane] = u0 + lane < a.nq ? PKEY_MAX : 0;            // rows past the end: nothing is ever below
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (a.filt_off && !use_bmg && !(a.dbg & 16)) {
    // (No bitmap of the pass -- it would not fit the scratch cap: every split's workgroup walks the lists itself.)
    // The 16 users of a wave are consecutive, so their filter lists are ONE contiguous run of the CSR ids: all 64 lanes walk it together
    // (sixteen independent loads in flight per lane) and find an entry's row by comparing its position with the 15 inner offsets.  (One list
    // after the other -- 48 dependent round trips -- was 18 of the sweep's 200 us, every split's workgroups repeating it; now 11.)
    const int64_t uo = u0 + (lane < 16 ? lane : 16);
    const int64_t myoff = a.filt_off[uo < a.nq ? uo : a.nq];
    const int64_t f_begin = __shfl(myoff, 0, 64), f_end = __shfl(myoff, 16, 64);
    uint32_t rel[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) rel[k] = (uint32_t)(__shfl(myoff, k + 1, 64) - f_begin);
    const int64_t span = i_hi - i_lo;
    constexpr int FB = 16;                                               // loads in flight per lane
    for (int64_t base = f_begin; base < f_end; base += 64 * FB) {
      int32_t ids[FB];
#pragma unroll
      for (int k = 0; k < FB; ++k) {
        const int64_t f = base + lane + 64 * k;
        ids[k] = f < f_end ? a.filt_ids[f] : -1;
      }
#pragma unroll
      for (int k = 0; k < FB; ++k) {
        const int64_t id = (int64_t)ids[k] - i_lo;
        const uint32_t pos = (uint32_t)(base - f_begin) + lane + 64 * k;
        int r = 0;
#pragma unroll
        for (int q = 0; q < 15; ++q) r += pos >= rel[q] ? 1 : 0;
        if (ids[k] >= 0 && id >= 0 && id < span) atomicOr(bm + r * a.bm_words + (id >> 5), 1u << (id & 31));
      }
    }
  }
  if (lane < 16) *reinterpret_cast<v4*>(usc + lane * 4) =
      u0 + lane < a.nq ? *reinterpret_cast<const v4*>(a.SCU + (u0 + lane) * 4) : (v4){0.f, 0.f, 0.f, 0.f};
  // A operands of the whole pass (user j): k-quad kq of every whole 16-block, then element kq of every remaining k-quad
  KTUP_Q_USER_OPS(G, u0 + j < a.nq && !(a.dbg & 32), a.A + (ok ? u0 + j : 0) * G::AROW, kq)
  if (use_bmg) {
    const int nw = 16 * a.bm_words;
#pragma unroll
    for (int k = 0; k < BMR; ++k)
      if (lane + 64 * k < nw) bm[lane + 64 * k] = bmv[k];
    for (int idx = lane + 64 * BMR; idx < nw; idx += 64) {                // (splits of more than 1024 items)
      const int r = idx / a.bm_words;
      bm[idx] = a.bmg[((u0 + r) * a.nsplit + sp) * a.bm_words + (idx - r * a.bm_words)];
    }
  }
  __syncthreads();                                                        // tiles zeroed, bitmaps and scalars in place
  const int64_t ntile = (a.dbg & 8) ? 0 : (i_hi - i_lo + IBT - 1) / IBT;    // (dbg 8: prologue and epilogue only)
  // this lane's float4 of every DMA piece of its wave: byte offset inside a tile (tiles past the table's end re-read its last row:
  // their items are masked out below, the operands only have to be finite)
  KTUP_Q_DMA_OFFSETS(G, soff, w, lane)
  auto dma = [&](int64_t t, int buf) {                                    // tile t of this split -> LDS buffer `buf`
    KTUP_Q_TILE_DMA(G, a.B, a.n_items, i_lo + t * IBT, Xb + buf * G::TILE_F4 + 64 * w, soff)
  };
  const int rowbase = 16 * kq;
  // A user's list is touched only when 16 candidates are pending for it.  A score is a candidate if it is below the user's n-th score
  // -- compared as FLOATS (thrf; NaN while the list is short: every score then takes the key compare below); equality or a NaN sends
  // the wave through the 64-bit key compare, so the order is that of the keys in every case.  Candidates are appended to the user's
  // pending row in LDS at positions taken from a ballot (no atomics; `pend` is replicated over the row's 16 lanes); once a row of a
  // register slot holds 16, that slot's four rows go through the merge network -- 16 real candidates per network pass instead of the
  // ~2 a tile yields -- and the thresholds are renewed.  (The network per tile and slot was 400 of this kernel's ~670 VALU
  // instructions per tile.)
  // The splits of a user share their bounds (a.gthr): any split's n-th score bounds the user's final n-th score from above, so a
  // score above it is no candidate anywhere (a split's list may then end short: the merge pads).  Published at every merge, re-read
  // once per tile -- requested before the tile's MFMAs (past the L1: the line changes under the kernel), used after them.  A stale
  // value is an older bound, never a wrong one.  With the XCD-aware mapping above a user's splits share one L2.  Each split alone
  // sends ~47 candidates per user through the append / merge path below, together ~4x fewer.
  float thrf[4];
  int pend[4] = {0, 0, 0, 0};
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) thrf[reg] = u0 + 4 * kq + reg < a.nq ? __uint_as_float(0x7fffffffu) : -__builtin_inff();
  const RowAppend app(kq, j);
  auto flush = [&](bool all) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int n = pend[reg];
      if (!__builtin_amdgcn_ballot_w64(all ? n > 0 : n >= 16)) continue;
      const int ur = 4 * kq + reg;
      const uint64_t* row = pbuf + ur * PCAP;
      uint64_t merged;                                                            // the segment that holds the n-th key
      if constexpr (SEG == 1) {
        merged = row_merge_pending(tk[ur * 16 + j], row, n, topn, j);             // all four rows of the slot at once
        tk[ur * 16 + j] = merged;
      } else {
        uint64_t* lst = tk + ur * 16 * SEG + j;                                   // element p = 16 s + j: key s of lane j
        uint64_t seg[SEG];
#pragma unroll
        for (int s = 0; s < SEG; ++s) seg[s] = lst[16 * s];
        row_merge_pending_wide<SEG>(seg, row, n, topn, j);
        merged = seg[0];
#pragma unroll
        for (int s = 0; s < SEG; ++s) {
          lst[16 * s] = seg[s];
          if (s == (topn - 1) >> 4) merged = seg[s];
        }
      }
      pend[reg] = 0;
      const int nj = SEG == 1 ? topn - 1 : (topn - 1) & 15;                       // the lane of the n-th key in its segment
      if (u0 + ur < a.nq) {                                                       // (rows past the end keep thrf = -inf, thrk = 0)
        const uint32_t hi = (uint32_t)__shfl((int)(merged >> 32), rowbase + nj, 64);
        const float own = topn_key_score(hi);                                     // (NaN: list short)
        thrf[reg] = own;                                                          // (the next tile's refresh brings the shared bound back)
        if (j == nj) {
          thrk[ur] = merged;
          // the splits of a user tell each other: non-negative floats order like their bits (a negative n-th score -- rounding of a
          // squared distance -- is published as 0: a weaker bound, still one)
          if (a.gthr && own == own) atomicMin(a.gthr + u0 + ur, __float_as_int(__builtin_fmaxf(own, 0.f)));
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto compute = [&](int buf, int sub, int64_t t, const int (&gl)[4]) {   // 16 users x the 16 items of tile t
    KTUP_Q_TILE_MFMA(G, Xb + buf * G::TILE_F4 + (sub * IBT + j) * ROW4, kq)   // lane (kq, item j) -> accAA, accS, accAN, accNN
    const v4 is4 = Xb[buf * G::TILE_F4 + (sub * IBT + j) * ROW4 + RB4];      // the row's scalars ride in its tile slot
    const int64_t item = i_lo + t * IBT + j;
    const int64_t lid = item - i_lo;
    const bool iok = item < i_hi;
    bool full = false;
    if (a.dbg & 1) {                                                       // measurement: keep the MFMAs alive, skip the ranking
      if (accS[0] + accAA[1] + accAN[2] + accNN[3] == 12345.f) thrf[0] = is4[0];
      return;
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int ur = 4 * kq + reg;
      // (as integers: gl is a non-negative float's bits or 0x7fffffff, and a bound of this split that is negative, -inf or a NaN of
      //  either sign keeps the meaning it has without the shared word)
      thrf[reg] = __int_as_float(min(__float_as_int(thrf[reg]), gl[reg]));
      const v4 us4 = *reinterpret_cast<const v4*>(usc + ur * 4);
      const float score = q_score(us4, is4, accS[reg], accAA[reg], accAN[reg], accNN[reg]);
      // one compare whose result stays a wave mask; with the shared bounds many 64-score slots have no candidate and leave here
      const uint64_t m_ngt = __builtin_amdgcn_ballot_w64(!(score > thrf[reg]));   // below the bound, equal to it, or unordered
      if (m_ngt == 0) continue;
      bool c = score < thrf[reg];
      if (m_ngt != __builtin_amdgcn_ballot_w64(c)) {                       // the keys decide (always while the list is short)
        if (!c && !(score > thrf[reg])) c = topn_key(score, false, (uint32_t)item) < thrk[ur];
      }
      c = c && iok;
      if (c) c = ((bm[ur * a.bm_words + (lid >> 5)] >> (lid & 31)) & 1u) == 0u;
      const uint64_t m = __builtin_amdgcn_ballot_w64(c);
      if (m) {
        app.put(pbuf, ur * PCAP, pend[reg], m, c, [&] { return topn_key(score, false, (uint32_t)item); });
        full |= pend[reg] >= 16;
      }
    }
    if (__builtin_amdgcn_ballot_w64(full)) flush(false);
  };
  if (ntile > 0) {
    if (!(a.dbg & 2)) dma(0, 0);
    __syncthreads();                                                       // (carries the vmcnt(0) that lands the DMA)
  }
  // one tile per workgroup barrier; the next tile's DMA is in flight under this tile's MFMAs.  Buffer buf ^ 1 was last read in the
  // previous iteration, whose closing barrier every wave has passed; its new contents are read after this iteration's barrier.
  for (int64_t t0 = 0; t0 < ntile; ++t0) {
    const int buf = (int)(t0 & 1);
    if (t0 + 1 < ntile && !(a.dbg & 2)) dma(t0 + 1, buf ^ 1);
    int gl[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
    if (a.gthr) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) gl[reg] = __hip_atomic_load(a.gthr + u0 + 4 * kq + reg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    compute((a.dbg & 2) ? 0 : buf, 0, t0, gl);
    if (!(a.dbg & 4)) __syncthreads();
  }
  flush(true);
  if constexpr (SEG == 1) {
    if (j < topn) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t ur = u0 + 4 * kq + reg;
        if (ur < a.nq) a.part[(ur * a.nsplit + sp) * topn + j] = tk[(4 * kq + reg) * 16 + j];
      }
    }
  } else {
#pragma unroll
    for (int s = 0; s < SEG; ++s) {
      const int p = 16 * s + j;                                            // this lane's key of segment s
      if (p >= topn) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t ur = u0 + 4 * kq + reg;
        if (ur < a.nq) a.part[(ur * a.nsplit + sp) * topn + p] = tk[(4 * kq + reg) * 16 * SEG + p];
      }
    }
  }
}

// G_RR | G_RN | G_NN, each [P4][P4] (zero padded), from the prepared tables (row pitch dp): one wave per entry.  gs (optional):
// the same numbers as the A operands of pspace_rows_mc_kernel's fold products, [matrix G_RR, G_RN, G_RN^T, G_NN][pt][k-step m][lane]
// with lane (k, i) <-> row 16 pt + 4 (i & 3) + (i >> 2), column 16 (m >> 2) + 4 (m & 3) + k; rows >= P4 are zero.
KTUP_DEV int gs_index(int mtx, int p, int q, int PT, int NP) {
  const int pt = p >> 4, pr = p & 15, i = (pr >> 2) + 4 * (pr & 3);
  const int m = (q >> 4) * 4 + ((q & 15) >> 2), k = q & 3;
  return ((mtx * PT + pt) * NP + m) * 64 + k * 16 + i;
}

__global__ __launch_bounds__(256) void pspace_gram_kernel(const float* __restrict__ Ar, const float* __restrict__ Cn, int dp, int d, int P, int P4,
                                                          float* __restrict__ grams, float* __restrict__ gs, int PT, int NP, FiltBm fb) {
  const int lane = threadIdx.x & 63;
  if ((int)blockIdx.x >= fb.gram_blocks) {                       // the pass's filter bitmap: four waves x 16 users per extra workgroup
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    filter_bitmap_wave(fb, ((int64_t)((int)blockIdx.x - fb.gram_blocks) * 4 + w) * 16,
                       reinterpret_cast<uint32_t*>(smem) + (size_t)w * 16 * fb.nsplit * fb.bm_words, lane);
    return;
  }
  const int gridx = fb.gram_blocks;
  for (int idx = blockIdx.x * 4 + (threadIdx.x >> 6); idx < 3 * P4 * P4; idx += gridx * 4) {
    const int t = idx / (P4 * P4), rem = idx - t * P4 * P4, p = rem / P4, q = rem - p * P4;
    float acc = 0.f;
    if (p < P && q < P) {
      const float* x = (t == 2 ? Cn : Ar) + (size_t)p * dp;
      const float* y = (t == 0 ? Ar : Cn) + (size_t)q * dp;
      for (int k = lane; k < d; k += 64) acc = fmaf(x[k], y[k], acc);
    }
    acc = group_sum<64>(acc);
    if (lane == 0) {
      grams[idx] = acc;
      if (gs) {
        if (t == 1) { gs[gs_index(1, p, q, PT, NP)] = acc; gs[gs_index(2, q, p, PT, NP)] = acc; }
        else gs[gs_index(t == 0 ? 0 : 3, p, q, PT, NP)] = acc;
      }
    }
  }
  if (gs && 16 * PT > P4)                                        // rows P4 .. 16 PT - 1 of the last row tile: zero
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < 4 * (16 * PT - P4) * P4; idx += gridx * 256) {
      const int mtx = idx / ((16 * PT - P4) * P4), rem = idx - mtx * (16 * PT - P4) * P4;
      gs[gs_index(mtx, P4 + rem / P4, rem % P4, PT, NP)] = 0.f;
    }
}

// One wave per row x (user: U[ids[row]]; item: X[row]): L = Alog x, Rx = Ar x, Nx = Cn x (lane = one of the 3 P4 table rows, the
// tables staged transposed in LDS), then the operand row and the four scalars of the formulation above.
struct RowsSide {
  const float* X; int64_t ldx; const int64_t* ids;   // rows X[ids[row]] (ids == NULL: X[row])
  const float* E; int64_t lde; const int32_t* map;    // + E[map[row]] (KTUP items: the aligned entity, the pad row being zero); NULL = none
  int64_t nrows; float* out; int orow; float* scal; int blocks;
  int opitch, spitch;                                 // floats between two rows of out / of scal (items: both G::GROW, scal = out + ROWB)
  int32_t* gthr;                                      // users: the sweep's shared n-th score per user, reset here (NULL: none / items)
};

template <bool IS_USER, int NCH, int NP>
KTUP_DEV void pspace_rows(const RowsSide& sd, int block, int P, const float* __restrict__ Alog, const float* __restrict__ Ar,
                          const float* __restrict__ Cn, int dp, const float* __restrict__ grams, int ka16, int ks16) {
  const float* __restrict__ X = sd.X;
  const int64_t ldx = sd.ldx, nrows = sd.nrows;
  const int64_t* __restrict__ ids = sd.ids;
  float* __restrict__ out = sd.out;
  float* __restrict__ scal = sd.scal;
  const int orow = sd.orow;
  constexpr int d = 4 * NCH, P4 = 4 * NP;                        // compile-time: the k loops unroll and their LDS reads batch
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // the tables (3 P x d floats = 24 KB at P = 20, d = 100) and the Gram matrices are read straight from global memory: they stay in
  // the CU's vector L1, and staging them in LDS per workgroup cost more than the rows' own work
  float* wv = lds;                                               // per wave: x [d] | res [3 P4] | fold [4 P4]
  constexpr int wstride = d + 7 * P4;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* G = grams;
  float* xs = wv + w * wstride;
  float* res = xs + d;
  float* fold = res + 3 * P4;
  for (int64_t row = (int64_t)block * 4 + w; row < nrows; row += (int64_t)sd.blocks * 4) {
    const float* x = X + (ids ? ids[row] : row) * ldx;
    const float* e = sd.E ? sd.E + (int64_t)sd.map[row] * sd.lde : nullptr;
    float sq = 0.f;
    for (int k = lane; k < d; k += 64) { const float v = e ? x[k] + e[k] : x[k]; xs[k] = v; sq = fmaf(v, v, sq); }
    sq = group_sum<64>(sq);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int col = lane; col < 3 * P4; col += 64) {
      const int t = col / P4, p = col - t * P4;
      float4 acc = f4zero();
      if (p < P) {
        const float4* tr = reinterpret_cast<const float4*>((t == 0 ? Alog : t == 1 ? Ar : Cn) + (size_t)p * dp);
        const float4* xr = reinterpret_cast<const float4*>(xs);
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc = acc + xr[c] * tr[c];
      }
      res[col] = (acc.x + acc.y) + (acc.z + acc.w);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const float* L = res;
    const float* Rx = res + P4;
    const float* Nx = res + 2 * P4;
    // Gram products of L: fold[0] = G_RR L, [1] = G_RN L, [2] = G_RN^T L, [3] = G_NN L; quadratic forms by wave sums
    float q_rr = 0.f, q_rn = 0.f, q_nn = 0.f, d_nl = 0.f, d_rl = 0.f;
    if (lane < P4) {
      float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
#pragma unroll
      for (int q = 0; q < P4; ++q) {
        const float lq = L[q];
        g0 = fmaf(G[lane * P4 + q], lq, g0);
        g1 = fmaf(G[P4 * P4 + lane * P4 + q], lq, g1);
        g2 = fmaf(G[P4 * P4 + q * P4 + lane], lq, g2);
        g3 = fmaf(G[2 * P4 * P4 + lane * P4 + q], lq, g3);
      }
      fold[lane] = g0; fold[P4 + lane] = g1; fold[2 * P4 + lane] = g2; fold[3 * P4 + lane] = g3;
      const float l = L[lane];
      q_rr = l * g0; q_rn = l * g1; q_nn = l * g3; d_nl = Nx[lane] * l; d_rl = Rx[lane] * l;
    }
    q_rr = group_sum<64>(q_rr); q_rn = group_sum<64>(q_rn); q_nn = group_sum<64>(q_nn);
    d_nl = group_sum<64>(d_nl); d_rl = group_sum<64>(d_rl);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float* o = out + row * (int64_t)sd.opitch;
    if (IS_USER) {
      // [AA: -2u ; -2L ; 2 (Ru + G_RR L) ; 0] [S: Nu ; -L ; 0] [AN: Nu + G_RN^T L + G_RN L ; -L ; 0] [NN: 2 G_NN L ; 0]
      const int oS = 16 * ka16, oAN = oS + 16 * ks16, oNN = oAN + 16 * ks16;
      for (int k = lane; k < orow; k += 64) {
        float v = 0.f;
        if (k < oS) {
          if (k < d) v = -2.f * xs[k];
          else if (k < d + P4) v = -2.f * L[k - d];
          else if (k < d + 2 * P4) v = 2.f * (Rx[k - d - P4] + fold[k - d - P4]);
        } else if (k < oAN) {
          const int e = k - oS;
          if (e < P4) v = Nx[e]; else if (e < 2 * P4) v = -L[e - P4];
        } else if (k < oNN) {
          const int e = k - oAN;
          if (e < P4) v = Nx[e] + fold[2 * P4 + e] + fold[P4 + e]; else if (e < 2 * P4) v = -L[e - P4];
        } else {
          const int e = k - oNN;
          if (e < P4) v = 2.f * fold[3 * P4 + e];
        }
        o[k] = v;
      }
      // u.NU, |AU|^2, AU.NU, |NU|^2
      if (lane == 0) *reinterpret_cast<float4*>(scal + row * (int64_t)sd.spitch) = make_float4(d_nl, sq + 2.f * d_rl + q_rr, d_nl + q_rn, q_nn);
      if (lane == 0 && sd.gthr) sd.gthr[row] = 0x7fffffff;
    } else {
      // [x ; Rx ; L ; Nx]
      for (int k = lane; k < orow; k += 64) o[k] = k < d ? xs[k] : k < d + P4 ? Rx[k - d] : k < d + 2 * P4 ? L[k - d - P4] : Nx[k - d - 2 * P4];
      // v.NV, |C0|^2, C0.NV, |NV|^2
      if (lane == 0) {
        *reinterpret_cast<float4*>(scal + row * (int64_t)sd.spitch) = make_float4(d_nl, sq - 2.f * d_rl + q_rr, d_nl - q_rn, q_nn);
        for (int k = orow + 4; k < sd.opitch; ++k) o[k] = 0.f;              // the pitch's spare float4 (padded K blocks may read it)
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// users and items in ONE launch: the first `users.blocks` workgroups take the user rows, the rest the item rows
template <int NCH, int NP>
__global__ __launch_bounds__(256) void pspace_rows_kernel(RowsSide users, RowsSide items, int P, const float* __restrict__ Alog,
                                                          const float* __restrict__ Ar, const float* __restrict__ Cn, int dp,
                                                          const float* __restrict__ grams, int ka16, int ks16) {
  if ((int)blockIdx.x < users.blocks) pspace_rows<true, NCH, NP>(users, blockIdx.x, P, Alog, Ar, Cn, dp, grams, ka16, ks16);
  else pspace_rows<false, NCH, NP>(items, blockIdx.x - users.blocks, P, Alog, Ar, Cn, dp, grams, ka16, ks16);
}

// The same rows on the matrix cores: a wave owns 16 rows.  L^T, Rx^T, Nx^T = (Alog | Ar | Cn) . x^T with the tables staged
// slot-ordered in LDS exactly as in pref_fwd_mc (lane (kq, j = row) ends up with preference 16 tt + 4 reg + kq of its row), the
// four Gram folds G_RR L, G_RN L, G_RN^T L, G_NN L as K = P products whose B operands are those registers (the Gram matrices
// staged in the matching slot / k order), the row scalars by lane-swap sums over the four kq lanes, and the operand rows written
// straight from the registers (16 B per (row, preference quad)).  One wave per row (above) is a chain of ~10 dependent round
// trips per row -- 31 us for the 9,746 rows of an ml1m pass; 16 rows per wave are ~210 MFMAs.
template <int NCH_, int NP_>
struct RGeom {
  static constexpr int NCH = NCH_, NP = NP_, D = 4 * NCH, P4 = 4 * NP;
  static constexpr int PT = (NP + 3) / 4, KG = (D + 15) / 16;
  static constexpr int PITCHA4 = 4 * KG + 1;
  static constexpr int SLOT_F4 = PT * 16 * PITCHA4;              // one table, float4
  static constexpr int GS_F = 4 * PT * NP * 64;                  // Gram A operands: [matrix][pt][k-step][lane]
  static constexpr int J = (16 * NCH + 63) / 64;
  static constexpr int TILE_F4 = 16 * NCH + 3;
  static constexpr size_t WAVE_BYTES = (size_t)TILE_F4 * 16 + 2 * 16 * 4;
  static constexpr size_t LDS = (size_t)3 * SLOT_F4 * 16 + (size_t)GS_F * 4 + 4 * WAVE_BYTES;
};

template <int NCH, int NP>
__global__ __launch_bounds__(256) void pspace_rows_mc_kernel(RowsSide users, RowsSide items, int P, const float* __restrict__ Alog,
                                                             const float* __restrict__ Ar, const float* __restrict__ Cn, int dp,
                                                             const float* __restrict__ gs, int ka16, int ks16, FiltBm fb) {
  using R = RGeom<NCH, NP>;
  constexpr int D = R::D, P4 = R::P4, PT = R::PT, KG = R::KG, PITCHA4 = R::PITCHA4, J = R::J;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if ((int)blockIdx.x >= users.blocks + items.blocks) {          // the pass's filter bitmap rides here: the walk is one wave's chain of
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // round trips (~10 us), as long as this launch and on CUs it leaves idle
    filter_bitmap_wave(fb, ((int64_t)((int)blockIdx.x - users.blocks - items.blocks) * 4 + wv) * 16,
                       reinterpret_cast<uint32_t*>(smem) + (size_t)wv * 16 * fb.nsplit * fb.bm_words, threadIdx.x & 63);
    return;
  }
  v4* Slot = reinterpret_cast<v4*>(smem);                         // [3][PT * 16 slots][PITCHA4]
  float* GS = reinterpret_cast<float*>(Slot + 3 * R::SLOT_F4);
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* wbase = reinterpret_cast<char*>(GS + R::GS_F) + (size_t)w * R::WAVE_BYTES;
  v4* XT = reinterpret_cast<v4*>(wbase);                          // x  [16][NCH] (+ 3 chunks never used unmasked)
  int32_t* sid = reinterpret_cast<int32_t*>(XT + R::TILE_F4);     // [2][16]
  const bool is_user = (int)blockIdx.x < users.blocks;
  const RowsSide& sd = is_user ? users : items;
  const int block = is_user ? (int)blockIdx.x : (int)blockIdx.x - users.blocks;
  const int64_t row0 = ((int64_t)block * 4 + w) * 16;
  const bool active = row0 < sd.nrows;
  const int orow = sd.orow;
  // the wave's rows are requested first; the tables are staged while they are on their way
  if (active && lane < 16) {
    const int64_t gr = row0 + lane;
    const bool ok = gr < sd.nrows;
    sid[lane] = ok ? (int32_t)(sd.ids ? sd.ids[gr] : gr) : 0;
    sid[16 + lane] = (ok && sd.E) ? sd.map[gr] : 0;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  v4 xv[J], ev[J];
  if (active) {
    const v4* X4 = reinterpret_cast<const v4*>(sd.X);
    const v4* E4 = reinterpret_cast<const v4*>(sd.E);
    const uint32_t ldx4 = (uint32_t)(sd.ldx >> 2), lde4 = (uint32_t)(sd.lde >> 2);
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
      const int e = lane + 64 * jj;
      const int r = e < 16 * NCH ? e / NCH : 0, c = e < 16 * NCH ? e % NCH : 0;
      xv[jj] = X4[(uint64_t)(uint32_t)sid[r] * ldx4 + (uint32_t)c];
      ev[jj] = E4 ? E4[(uint64_t)(uint32_t)sid[16 + r] * lde4 + (uint32_t)c] : (v4){0.f, 0.f, 0.f, 0.f};
    }
  }
  {   // every load of the staging is issued before the first LDS write (a loop of load -> write round trips cost 6 us here)
    const v4 zero = (v4){0.f, 0.f, 0.f, 0.f};
    constexpr int SIT = (R::SLOT_F4 + 255) / 256, GIT = (R::GS_F / 4 + 255) / 256;
    v4 ta[SIT], tr[SIT], tc[SIT], tg[GIT];
#pragma unroll
    for (int it = 0; it < SIT; ++it) {
      const int idx = tid + 256 * it;
      const int srow = idx / PITCHA4, c = idx - srow * PITCHA4;
      const int tt = srow >> 4, i = srow & 15;
      const int p = 16 * tt + 4 * (i & 3) + (i >> 2);             // slot -> preference (block transposed, as in pref_fwd_mc)
      const bool ok = idx < R::SLOT_F4 && p < P && c < NCH;
      ta[it] = ok ? *reinterpret_cast<const v4*>(Alog + (size_t)p * dp + 4 * c) : zero;
      tr[it] = ok ? *reinterpret_cast<const v4*>(Ar + (size_t)p * dp + 4 * c) : zero;
      tc[it] = ok ? *reinterpret_cast<const v4*>(Cn + (size_t)p * dp + 4 * c) : zero;
    }
    const v4* g4 = reinterpret_cast<const v4*>(gs);               // already in operand order (pspace_gram_kernel)
#pragma unroll
    for (int it = 0; it < GIT; ++it) tg[it] = tid + 256 * it < R::GS_F / 4 ? g4[tid + 256 * it] : zero;
#pragma unroll
    for (int it = 0; it < SIT; ++it) {
      const int idx = tid + 256 * it;
      if (idx < R::SLOT_F4) { Slot[idx] = ta[it]; Slot[R::SLOT_F4 + idx] = tr[it]; Slot[2 * R::SLOT_F4 + idx] = tc[it]; }
    }
#pragma unroll
    for (int it = 0; it < GIT; ++it)
      if (tid + 256 * it < R::GS_F / 4) reinterpret_cast<v4*>(GS)[tid + 256 * it] = tg[it];
  }
  if (active) {
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
      const int e = lane + 64 * jj;
      if (e < 16 * NCH) {
        const int r = e / NCH, c = e % NCH;
        const v4 v = xv[jj] + ev[jj];
        XT[e] = v;
        if (row0 + r < sd.nrows)                                  // the x part of the operand row: [-2u ...] | [x ...]
          *reinterpret_cast<v4*>(sd.out + (row0 + r) * (int64_t)sd.opitch + 4 * c) = is_user ? -2.f * v : v;
      }
    }
  }
  __syncthreads();
  if (!active) return;
  // ---- L^T, Rx^T, Nx^T: acc[t][tt][reg] of lane (kq, row j) = table t's product for preference 16 tt + 4 reg + kq
  v4 acc[3][PT];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int tt = 0; tt < PT; ++tt) acc[t][tt] = (v4){0.f, 0.f, 0.f, 0.f};
  float sq = 0.f;
#pragma unroll
  for (int g = 0; g < KG; ++g) {
    v4 bv = XT[j * NCH + 4 * g + kq];
    if (4 * g + 3 >= NCH) {
      if (4 * g + kq >= NCH) bv = (v4){0.f, 0.f, 0.f, 0.f};
    }
    sq += (bv[0] * bv[0] + bv[1] * bv[1]) + (bv[2] * bv[2] + bv[3] * bv[3]);
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int tt = 0; tt < PT; ++tt) {
        const v4 av = Slot[t * R::SLOT_F4 + (tt * 16 + j) * PITCHA4 + 4 * g + kq];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[t][tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], bv[c], acc[t][tt], 0, 0, 0);
      }
  }
  sq = allsum_kq(sq);
  // ---- Gram folds: fold[0] = G_RR L, [1] = G_RN L, [2] = G_RN^T L, [3] = G_NN L   (same lane layout as L)
  v4 fold[4][PT];
#pragma unroll
  for (int mtx = 0; mtx < 4; ++mtx)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      fold[mtx][pt] = (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int m = 0; m < NP; ++m)
        fold[mtx][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(GS[((mtx * PT + pt) * NP + m) * 64 + lane], acc[0][m >> 2][m & 3], fold[mtx][pt], 0, 0, 0);
    }
  float q_rr = 0.f, q_rn = 0.f, q_nn = 0.f, d_nl = 0.f, d_rl = 0.f;
#pragma unroll
  for (int tt = 0; tt < PT; ++tt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float l = acc[0][tt][reg];
      q_rr = fmaf(l, fold[0][tt][reg], q_rr); q_rn = fmaf(l, fold[1][tt][reg], q_rn); q_nn = fmaf(l, fold[3][tt][reg], q_nn);
      d_nl = fmaf(acc[2][tt][reg], l, d_nl); d_rl = fmaf(acc[1][tt][reg], l, d_rl);
    }
  q_rr = allsum_kq(q_rr); q_rn = allsum_kq(q_rn); q_nn = allsum_kq(q_nn); d_nl = allsum_kq(d_nl); d_rl = allsum_kq(d_rl);
  const int64_t row = row0 + j;
  if (row >= sd.nrows) return;
  float* o = sd.out + row * (int64_t)sd.opitch;
  if (is_user) {
    // [AA: -2u ; -2L ; 2 (Ru + G_RR L) ; 0] [S: Nu ; -L ; 0] [AN: Nu + G_RN^T L + G_RN L ; -L ; 0] [NN: 2 G_NN L ; 0]
    const int oS = 16 * ka16, oAN = oS + 16 * ks16, oNN = oAN + 16 * ks16;
#pragma unroll
    for (int tt = 0; tt < PT; ++tt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int p = 16 * tt + 4 * reg + kq;
        if (p < P4) {
          const float l = acc[0][tt][reg], rx = acc[1][tt][reg], nx = acc[2][tt][reg];
          o[D + p] = -2.f * l;
          o[D + P4 + p] = 2.f * (rx + fold[0][tt][reg]);
          o[oS + p] = nx;
          o[oS + P4 + p] = -l;
          o[oAN + p] = nx + fold[2][tt][reg] + fold[1][tt][reg];
          o[oAN + P4 + p] = -l;
          o[oNN + p] = 2.f * fold[3][tt][reg];
        }
      }
    for (int k = D + 2 * P4 + kq; k < oS; k += 4) o[k] = 0.f;
    for (int k = oS + 2 * P4 + kq; k < oAN; k += 4) o[k] = 0.f;
    for (int k = oAN + 2 * P4 + kq; k < oNN; k += 4) o[k] = 0.f;
    for (int k = oNN + P4 + kq; k < orow; k += 4) o[k] = 0.f;
    // u.NU, |AU|^2, AU.NU, |NU|^2
    if (kq == 0) *reinterpret_cast<float4*>(sd.scal + row * (int64_t)sd.spitch) = make_float4(d_nl, sq + 2.f * d_rl + q_rr, d_nl + q_rn, q_nn);
    if (kq == 0 && sd.gthr) sd.gthr[row] = 0x7fffffff;
  } else {
    // [x ; Rx ; L ; Nx]
#pragma unroll
    for (int tt = 0; tt < PT; ++tt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int p = 16 * tt + 4 * reg + kq;
        if (p < P4) {
          o[D + p] = acc[1][tt][reg];
          o[D + P4 + p] = acc[0][tt][reg];
          o[D + 2 * P4 + p] = acc[2][tt][reg];
        }
      }
    // v.NV, |C0|^2, C0.NV, |NV|^2
    if (kq == 0) {
      *reinterpret_cast<float4*>(sd.scal + row * (int64_t)sd.spitch) = make_float4(d_nl, sq - 2.f * d_rl + q_rr, d_nl - q_rn, q_nn);
      for (int k = orow + 4; k < sd.opitch; ++k) o[k] = 0.f;                // the pitch's spare float4 (padded K blocks may read it)
    }
  }
}

struct QScratch { float *grams, *gs, *A, *SCU, *B; uint64_t* part; uint32_t* bm; int32_t* gthr; };

// Words of the pass's filter bitmap per user for ANY split count <= 8 (nsplit x ceil(split_items / 32) with split_items = 16 x
// ceil(tiles / nsplit)), and the cap under which the pass builds one (beyond it every split's workgroup walks the CSR lists itself)
inline size_t filt_bm_words_per_user(int64_t n_items) { return (size_t)((n_items + IBT - 1) / IBT) / 2 + 13; }
inline size_t filt_bm_bytes(int64_t nq, int64_t n_items) {
  const size_t b = (size_t)((nq + 63) / 64) * 64 * filt_bm_words_per_user(n_items) * sizeof(uint32_t);
  return b <= ((size_t)128 << 20) ? b : 0;
}

// Catalogue splits a pass may use and the keys of a user's partial lists in the scratch: the narrow entry keeps 8 splits x TOPN_MAX
// whatever topn is; the wide one sizes them by topn, with at most 512 / topn splits (what topk_merge_kernel<8, .> holds) and 8.
inline int q_max_splits(int topn, bool wide) { return wide && 512 / topn < 8 ? 512 / topn : 8; }
inline size_t q_part_keys(int topn, bool wide) { return wide ? (size_t)q_max_splits(topn, true) * topn : (size_t)8 * TOPN_MAX; }

template <typename G>
QScratch q_carve(void* scratch, int64_t nq, int64_t n_items, size_t part_keys) {
  QScratch s;
  float* p = reinterpret_cast<float*>(scratch);
  s.grams = p; p += 3 * 32 * 32;
  s.gs = p; p += 4 * 2 * 8 * 64;                                 // RGeom::GS_F at its largest (PT = 2, NP = 8)
  s.A = p; p += (size_t)nq * G::AROW;
  s.SCU = p; p += (size_t)nq * 4;
  s.B = p; p += (size_t)n_items * G::GROW + 64;                  // (eval_pass_pspace_bytes counts the same)
  s.part = reinterpret_cast<uint64_t*>(p);
  s.gthr = reinterpret_cast<int32_t*>(s.part + (size_t)nq * part_keys);     // (eval_pass_pspace_bytes: nq x q_part_keys)
  s.bm = reinterpret_cast<uint32_t*>(s.gthr + ((nq + 63) / 64) * 64);
  return s;
}

// The operand tables of a pass, for the list passes (launch_q) and the rank pass (pref_q_tables below; ktup_pref_rank_pass.hip): the
// Gram launch and the operand-row launch, with the filter bitmap's waves riding in one of them where the caller has one (use_bm; fb
// always names the Gram workgroups).  ONE rule for rows_mc -- the two row kernels round differently, and the ranks are counts against
// the list pass's own bits.  gthr: the users' shared bounds the row launch resets (NULL: none).
// The two row kernels come as ARGUMENTS (q_row_kernels<G>() at the call): a translation unit's kernels are emitted in the order its
// host code first names them, and launch_q names them before its sweep kernel as it did when these launches stood in its own body
// -- so the object's kernels keep their order and the file compares equal line by line (profiles/pref_ranks_narrow_check.txt).
using RowsMcKernel = void (*)(RowsSide, RowsSide, int, const float*, const float*, const float*, int, const float*, int, int, FiltBm);
using RowsKernel = void (*)(RowsSide, RowsSide, int, const float*, const float*, const float*, int, const float*, int, int);
struct RowKernels { RowsMcKernel mc; RowsKernel row; };                 // mc == NULL: no matrix-core row kernel at this geometry
// d = 256: the three staged tables + the Gram operands + four wave tiles of the matrix-core row kernel pass the LDS of a CU at P > 4
// (RGeom<64, 5>::LDS = 176 KB, <64, 8> 182 KB; <64, 1> 118 KB fits): those take the one-wave-per-row kernel, which stages nothing
template <typename G>
RowKernels q_row_kernels() {
  RowKernels k{nullptr, nullptr};
  if constexpr (RGeom<G::NCH, G::NP>::LDS <= 160 * 1024) k.mc = pspace_rows_mc_kernel<G::NCH, G::NP>;
  k.row = pspace_rows_kernel<G::NCH, G::NP>;
  return k;
}

template <typename G>
int q_tables(const RowKernels& kern, const float* U, int64_t ldu, const int64_t* u_ids, int64_t nq, const float* I, int64_t ldi, const float* E,
             int64_t lde, const int32_t* item2ent, int64_t n_items, const float* pref_ws, int ppad, int dp, int n_pref, const QScratch& q,
             int32_t* gthr, const FiltBm& fb, bool use_bm, size_t bm_lds, hipStream_t st, const char* name) {
  const float* Alog = pref_ws;
  const float* Ar = pref_ws + (size_t)ppad * dp;
  const float* Cn = pref_ws + (size_t)(ppad + n_pref) * dp;
  using R = RGeom<G::NCH, G::NP>;
  const bool rows_mc = kern.mc && opt_eval_mc() && !((ldu | ldi | lde | dp) & 3) && aligned16(U) && aligned16(I) && (!E || aligned16(E)) &&
                       aligned16(pref_ws) && nq < (1ll << 31) && n_items < (1ll << 31);
  const int64_t ublocks = (nq + 63) / 64;
  // the bitmap's waves ride in the operand-row launch (16 us, 146 workgroups at ml1m size); without the matrix-core row kernel, in the Gram launch
  const bool bm_in_gram = use_bm && !rows_mc;
  hipLaunchKernelGGL(pspace_gram_kernel, dim3(fb.gram_blocks + (bm_in_gram ? (unsigned)ublocks : 0u)), dim3(256), bm_in_gram ? bm_lds : 0, st, Ar, Cn, dp,
                     G::D, n_pref, G::P4, q.grams, rows_mc ? q.gs : nullptr, R::PT, G::NP, fb);
  const size_t lds_rows = (size_t)4 * (G::D + 7 * G::P4) * sizeof(float);
  // many small workgroups: a row is a chain of dependent round trips (id -> row -> products -> store), hidden only by occupancy
  RowsSide us{U, ldu, u_ids, nullptr, 0, nullptr, nq, q.A, G::AROW, q.SCU, grid_for((nq + 3) / 4, 2048), G::AROW, 4, gthr};
  RowsSide is{I, ldi, nullptr, E, lde, item2ent, n_items, q.B, G::ROWB, q.B + G::ROWB, grid_for((n_items + 3) / 4, 2048), G::GROW, G::GROW, nullptr};
  if (rows_mc) {    // 16 rows per wave on the matrix cores
    us.blocks = (int)((nq + 63) / 64); is.blocks = (int)((n_items + 63) / 64);
    const size_t rows_lds = use_bm && bm_lds > R::LDS ? bm_lds : R::LDS;
    (void)hipFuncSetAttribute((const void*)kern.mc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rows_lds);
    hipLaunchKernelGGL(kern.mc, dim3(us.blocks + is.blocks + (use_bm ? (unsigned)ublocks : 0u)), dim3(256), rows_lds, st, us, is, n_pref, Alog, Ar, Cn,
                       dp, q.gs, G::KA, G::KS, fb);
  } else {
    hipLaunchKernelGGL(kern.row, dim3(us.blocks + is.blocks), dim3(256), lds_rows, st, us, is, n_pref, Alog, Ar, Cn, dp, q.grams, G::KA, G::KS);
  }
  return check_launch(name);
}

// SEG = 1: the narrow entry point's pass.  SEG = 2, 4: the wide one's (topn <= 16 SEG).
template <typename G, int SEG = 1>
int launch_q(const float* U, int64_t ldu, const int64_t* u_ids, int64_t nq, const float* I, int64_t ldi, const float* E, int64_t lde,
             const int32_t* item2ent, int64_t n_items, const float* pref_ws,
             int ppad, int dp, int n_pref, const int64_t* filt_off, const int32_t* filt_ids, int topn, void* scratch, int32_t* top_ids,
             float* top_scores, hipStream_t st, const char* name) {
  constexpr bool WIDE = SEG > 1;
  const QScratch q = q_carve<G>(scratch, nq, n_items, q_part_keys(topn, WIDE));
  // the catalogue splits of the sweep (decided here: the filter bitmap is laid out by split)
  const int64_t ublocks = (nq + 63) / 64;
  const int max_splits = q_max_splits(topn, WIDE);
  const int64_t tiles = (n_items + IBT - 1) / IBT;
  int nsplit, bm_words;
  int64_t split_items;
  size_t lds;
  auto plan = [&](int resident) {                                         // `resident` workgroups per CU: ONE round
    nsplit = (int)(256 * resident / ublocks);
    if (nsplit > max_splits) nsplit = max_splits;
    if (opt_eval_nsplit() > 0 && opt_eval_nsplit() <= max_splits) nsplit = opt_eval_nsplit();   // measurement knob
    if (nsplit > tiles) nsplit = (int)tiles;
    if (nsplit < 1) nsplit = 1;
    split_items = ((tiles + nsplit - 1) / nsplit) * IBT;
    nsplit = (int)((n_items + split_items - 1) / split_items);
    bm_words = (int)((split_items + 31) / 32);
    lds = (size_t)2 * G::TILE_F4 * 16 + 4 * wave_lds_bytes<SEG>(bm_words);
  };
  plan(q_wgs<G, SEG>());                                                  // (narrow: MINW, what the registers allow)
  if (WIDE && 2 * lds > 160 * 1024) {
    // the wide lists and this catalogue's filter bits leave room for one workgroup per CU: split for one, if the longer splits'
    // filter bits still fit
    const int ns = nsplit, bw = bm_words;
    const int64_t si = split_items;
    const size_t l = lds;
    plan(1);
    if (lds > 160 * 1024) { nsplit = ns; bm_words = bw; split_items = si; lds = l; }
  }
  if (lds > 160 * 1024) return 1;
  const int gram_blocks = (3 * G::P4 * G::P4 + 3) / 4;
  const size_t bm_lds = (size_t)4 * 16 * nsplit * bm_words * sizeof(uint32_t);
  const bool use_bm = filt_off && filt_ids && filt_bm_bytes(nq, n_items) && (size_t)nsplit * bm_words <= filt_bm_words_per_user(n_items) &&
                      bm_lds <= 64 * 1024;
  FiltBm fb{filt_off, filt_ids, nq, n_items, q.bm, nsplit, bm_words, (uint32_t)split_items, gram_blocks};
  if (int e = q_tables<G>(q_row_kernels<G>(), U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, n_pref, q, q.gthr, fb, use_bm, bm_lds, st, name))
    return e;
  QArgs a{};
  a.A = q.A; a.SCU = q.SCU; a.B = q.B; a.nq = nq; a.n_items = n_items;
  a.filt_off = filt_off; a.filt_ids = filt_ids; a.topn = topn; a.part = q.part; a.dbg = opt_dbg_eval();
  a.split_items = split_items; a.nsplit = nsplit; a.bm_words = bm_words; a.bmg = use_bm ? q.bm : nullptr;
  a.gthr = nsplit > 1 && !(a.dbg & 64) ? q.gthr : nullptr;
  (void)hipFuncSetAttribute((const void*)eval_pass_q_kernel<G, SEG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((eval_pass_q_kernel<G, SEG>), dim3((unsigned)ublocks, (unsigned)nsplit), dim3(256), lds, st, a);
  if (int e = check_launch(name)) return e;
  return launch_topk_merge(q.part, nq, nsplit, topn, WIDE, top_ids, top_scores, st, name);   // nsplit x topn <= 128 (narrow) / 512 keys per user
}

// the rank pass's tables: Gram matrices and operand rows in the head of the list pass's scratch layout, no partial lists, bounds or bitmap
template <typename G>
int q_tables_only(const float* U, int64_t ldu, const int64_t* u_ids, int64_t nq, const float* I, int64_t ldi, const float* E, int64_t lde,
                  const int32_t* item2ent, int64_t n_items, const float* pref_ws, int ppad, int dp, int n_pref, void* scratch, PrefQTables* out,
                  hipStream_t st, const char* name) {
  const QScratch q = q_carve<G>(scratch, nq, n_items, 0);
  const FiltBm fb{nullptr, nullptr, nq, n_items, nullptr, 1, 0, 0u, (3 * G::P4 * G::P4 + 3) / 4};
  out->A = q.A; out->SCU = q.SCU; out->B = q.B;
  return q_tables<G>(q_row_kernels<G>(), U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, n_pref, q, nullptr, fb, false, 0, st,
                     name);
}

template <int NCH, int SEG>
int launch_q_p(int n_pref, const float* U, int64_t ldu, const int64_t* u_ids, int64_t nq, const float* I, int64_t ldi, const float* E,
               int64_t lde, const int32_t* item2ent, int64_t n_items,
               const float* pref_ws, int ppad, int dp, const int64_t* filt_off, const int32_t* filt_ids, int topn, void* scratch,
               int32_t* top_ids, float* top_scores, hipStream_t st, const char* name) {
  if (n_pref <= 4)
    return launch_q<QGeom<NCH, 1>, SEG>(U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, n_pref, filt_off, filt_ids, topn, scratch, top_ids, top_scores, st, name);
  if (n_pref <= 20)
    return launch_q<QGeom<NCH, 5>, SEG>(U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, n_pref, filt_off, filt_ids, topn, scratch, top_ids, top_scores, st, name);
  return launch_q<QGeom<NCH, 8>, SEG>(U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, n_pref, filt_off, filt_ids, topn, scratch, top_ids, top_scores, st, name);
}

template <int SEG>
int launch_q_d(int d, int n_pref, const float* U, int64_t ldu, const int64_t* u_ids, int64_t nq, const float* I, int64_t ldi, const float* E,
               int64_t lde, const int32_t* item2ent, int64_t n_items,
               const float* pref_ws, int ppad, int dp, const int64_t* filt_off, const int32_t* filt_ids, int topn, void* scratch,
               int32_t* top_ids, float* top_scores, hipStream_t st, const char* name) {
  if (d == 64) return launch_q_p<16, SEG>(n_pref, U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, filt_off, filt_ids, topn, scratch, top_ids, top_scores, st, name);
  if (d == 256) return launch_q_p<64, SEG>(n_pref, U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, filt_off, filt_ids, topn, scratch, top_ids, top_scores, st, name);
  if (d == 100) return launch_q_p<25, SEG>(n_pref, U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, filt_off, filt_ids, topn, scratch, top_ids, top_scores, st, name);
  return launch_q_p<32, SEG>(n_pref, U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, filt_off, filt_ids, topn, scratch, top_ids, top_scores, st, name);
}

}  // namespace

}  // namespace ktup

namespace ktup {

// the merge of the splits' partial lists, for this pass and the other sweeps (ktup_eval.hip: the soft and the hard gate's passes).
// Narrow: nsplit x topn <= 8 x 16 keys per user, two per lane; wide: <= 512, eight per lane.
int launch_topk_merge(const uint64_t* part, int64_t nq, int nsplit, int topn, bool wide, int32_t* top_ids, float* top_scores, hipStream_t st,
                      const char* name) {
  if (wide)
    hipLaunchKernelGGL((topk_merge_kernel<8, false>), dim3((unsigned)((nq + 3) / 4)), dim3(MERGE_T), 0, st, part, nq, nsplit, topn, top_ids,
                       top_scores);
  else
    hipLaunchKernelGGL((topk_merge_kernel<2, false>), dim3((unsigned)((nq + 3) / 4)), dim3(MERGE_T), 0, st, part, nq, nsplit, topn, top_ids,
                       top_scores);
  return check_launch(name);
}

// The preference-space pass (see QGeom): scratch for the Gram matrices, both operand tables, the scalars and the partial lists
// (narrow: 8 x TOPN_MAX keys per user whatever topn is; wide: q_part_keys, by topn).
size_t eval_pass_pspace_bytes(int d, int n_pref, int64_t nq, int64_t n_items, int topn, bool wide) {
  const size_t p4 = n_pref <= 4 ? 4 : n_pref <= 20 ? 20 : 32;
  const size_t ka = (d + 2 * p4 + 15) / 16, ks = (2 * p4 + 15) / 16, kn = (p4 + 15) / 16;
  const size_t arow = 16 * (ka + 2 * ks + kn), rowb = d + 3 * p4, grow = 4 * ((rowb / 4 + 1) | 1);      // QGeom::AROW, ROWB, GROW
  return (3 * 32 * 32 + 4 * 2 * 8 * 64 + (size_t)nq * (arow + 4) + (size_t)n_items * grow + 64) * sizeof(float) +
         (size_t)nq * q_part_keys(topn, wide) * sizeof(uint64_t) + (size_t)((nq + 63) / 64) * 64 * sizeof(int32_t) + filt_bm_bytes(nq, n_items);
}

// Items: I[row] (+ E[item2ent[row]] for KTUP; E == NULL for TUP); pref_ws: the prepared tables (ktup_pref_prepare; ppad / dp its
// geometry).  Returns KTUP_OK / an error, or 1 for shapes the pass does not cover.  wide: lists of two (topn <= 32) or four 16-key
// segments for 1 <= topn <= TOPN_WIDE_MAX; the scores are the narrow pass's bits.
int eval_pass_pspace(const float* U, int64_t ldu, const int64_t* u_ids, int64_t nq, const float* I, int64_t ldi, const float* E, int64_t lde,
                     const int32_t* item2ent, int64_t n_items, const float* pref_ws,
                     int ppad, int dp, int n_pref, int d, const int64_t* filt_off, const int32_t* filt_ids, int topn, void* scratch,
                     int32_t* top_ids, float* top_scores, hipStream_t st, const char* name, bool wide) {
  if ((d != 64 && d != 100 && d != 128 && d != 256) || n_pref < 1 || n_pref > 32 || topn < 1 || topn > (wide ? TOPN_WIDE_MAX : TOPN_MAX) ||
      n_items >= (1ll << 31))
    return 1;
  if (!wide) return launch_q_d<1>(d, n_pref, U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, filt_off, filt_ids, topn, scratch, top_ids, top_scores, st, name);
  if (topn <= 32) return launch_q_d<2>(d, n_pref, U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, filt_off, filt_ids, topn, scratch, top_ids, top_scores, st, name);
  return launch_q_d<4>(d, n_pref, U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, filt_off, filt_ids, topn, scratch, top_ids, top_scores, st, name);
}

// The operand tables alone, for the rank pass (ktup_pref_rank_pass.hip; defined after the list passes' entry so that their kernels are
// named first): `scratch` of pref_q_tables_bytes bytes, 16-byte aligned; *out:
// where the user rows, their scalars and the item rows are.  d in {64, 100, 128}, 1 <= n_pref <= 32 (the caller checked).
size_t pref_q_tables_bytes(int d, int n_pref, int64_t nq, int64_t n_items) {
  const size_t p4 = n_pref <= 4 ? 4 : n_pref <= 20 ? 20 : 32;
  const size_t ka = (d + 2 * p4 + 15) / 16, ks = (2 * p4 + 15) / 16, kn = (p4 + 15) / 16;
  const size_t arow = 16 * (ka + 2 * ks + kn), rowb = d + 3 * p4, grow = 4 * ((rowb / 4 + 1) | 1);      // QGeom::AROW, ROWB, GROW
  return (3 * 32 * 32 + 4 * 2 * 8 * 64 + (size_t)nq * (arow + 4) + (size_t)n_items * grow + 64) * sizeof(float);
}
int pref_q_tables(const float* U, int64_t ldu, const int64_t* u_ids, int64_t nq, const float* I, int64_t ldi, const float* E, int64_t lde,
                  const int32_t* item2ent, int64_t n_items, const float* pref_ws, int ppad, int dp, int n_pref, int d, void* scratch,
                  PrefQTables* out, hipStream_t st, const char* name) {
  auto by_p = [&](auto nch) {
    constexpr int NCH = decltype(nch)::value;
    if (n_pref <= 4)
      return q_tables_only<QGeom<NCH, 1>>(U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, n_pref, scratch, out, st, name);
    if (n_pref <= 20)
      return q_tables_only<QGeom<NCH, 5>>(U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, n_pref, scratch, out, st, name);
    return q_tables_only<QGeom<NCH, 8>>(U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, ppad, dp, n_pref, scratch, out, st, name);
  };
  if (d == 64) return by_p(std::integral_constant<int, 16>{});
  if (d == 100) return by_p(std::integral_constant<int, 25>{});
  return by_p(std::integral_constant<int, 32>{});
}

}  // namespace ktup
