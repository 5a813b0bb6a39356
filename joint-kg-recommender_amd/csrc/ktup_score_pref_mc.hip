// K5-K7 forward, soft gate, compile-time geometry: the matrix-core kernel for the common embedding sizes.
//
// Reference path: jTransUP/models/transUP.py:69-82,105-115 (TUP) and jTransUP/models/jTransUP.py:122-143,250-262 (KTUP):
//   x = u + i (+ e),  logits = x . A^T,  r = logits . Ar,  n = logits . Cn,  q = u - i (- e),
//   score = sum_k dist( q + r - (q . n) n )_k         (A, Ar, Cn: the mixed / pre-scaled tables of ktup_pref_prepare)
//
// Formulation (same as pref_fwd4 in ktup_score_pref.hip): a wave owns 16 pairs; logits^T = A . x^T and then
// r^T = Ar^T . logits^T, n^T = Cn^T . logits^T on v_mfma_f32_16x16x4_f32, pairs along the MFMA columns, so that the
// stage-1 accumulators ARE the stage-2 B operands.
//
// Why a second kernel: measurements on MI355X (tools/coissue_bench.hip, tools/valu_rate_bench.hip, profiles/) show that
// fp32 MFMA and VALU instructions do NOT overlap on a gfx950 SIMD -- not inside a wave, not across waves -- so this
// kernel's time is (MFMA passes + VALU instructions + exposed memory).  pref_fwd4 spends ~4000 clk per tile in MFMA
// and ~3500 clk in address arithmetic, bounds checks and scalar float4 math, because its geometry is run-time data.
// Here everything about the geometry is a template constant:
//   * gather: (row, chunk) of each of a lane's J loads is loop invariant and the ids are read from LDS with immediate offsets.
//     Through 64-bit pointers a load group (one row of each of the three tables) still compiles to 11 instructions on 64-bit
//     pairs (three v_mad_u64_u32, six v_lshl_add_u64, a shift, moves: the fences that keep the kernel inside 128 VGPRs also keep
//     the chunk offset from folding); with BUF (below) it is one v_add_u32 per load;
//   * all LDS operand addresses are one base register + immediates; no bounds checks in the matrix phases;
//   * x / q / distance math on <4 x float> values -> v_pk_add_f32 / v_pk_fma_f32;
//   * when the last 16-slot preference tile holds <= 4 preferences (P = 20), its logits come from
//     v_mfma_f32_4x4x1_16B_f32 (16 blocks = 4 pair groups x 4 k-quarters, 8 clk each) instead of a 3/4-empty 16x16x4.
//
// Split stage 2 (McGeom<.., SPLIT = true>, option fwd_split, soft gate, d <= 128): the two contractions over the preferences,
// r^T = Ar^T . logits^T and n^T = Cn^T . logits^T, are most of the fp32 MFMA clocks of a tile (2 NP 32-clock instructions per
// 16-coordinate tile).  They run on v_mfma_f32_16x16x32_bf16 instead (16 clk, K = 32 preference slots in one instruction) with
// fp32-grade products: both operands are split into three bf16 pieces hi + mid + lo == x (exactly), every bf16 x bf16 product is exact
// in the fp32 accumulator, and the six products hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi keep every term above 2^-24 of the full
// product -- 6 x 16 clk per tile and table whatever P is, against NP x 32.
//   * tables: Cn and Ar are split ONCE per workgroup while they are staged, into three bf16 planes each, [coordinate][k-quarter][8 slots]:
//     lane (kq, j) reads the A operand A[row = coordinate 16 ct + j][k = 8 kq + s] of a piece as one ds_read_b128.  The fp32 copies of
//     the two tables are not staged at all;
//   * logits: slot k = 8 kq + s is preference 4 s + kq = the logit register lg[s >> 2][s & 3] lane (kq, pair) holds after stage 1 (which
//     stays on the fp32 pipe: three bf16 planes of the x tile per wave do not fit the LDS), so the B operand is split in registers
//     (v_cvt_pk_bf16_f32 + a subtraction per level) and never passes through the LDS;
//   * C / D of the 16x16x32 form is laid out like the fp32 form's (row = 4 kq + reg, column = pair): the epilogue (s = q . n,
//     q + r - s n, the distance) is the fp32 kernel's, and accR still starts at q;
//   * d = 100: the last 4 coordinates are a seventh (mostly zero) tile instead of the fp32 kernel's 4x4x1 blocks + reduce-scatter.
// Used where it is fewer matrix clocks (NP >= 4) and the planes (3 x 64 B per coordinate and table) leave the workgroup as many waves
// as the fp32 tables: d = 64 (8 < P <= 32), d = 100 (8 < P <= 20), d = 128 (16 < P <= 20).  fwd_split = 0 runs the fp32 stage 2 everywhere.
//
// Packed split stage 2 (McGeom<.., SPLIT_PACK>, option fwd_split_pack, wherever the six-product form applies with P <= 20): a lane holds
// NS <= 5 logits, so slots 5-7 of every k-quarter multiply zeros in all six MFMAs above.  The 6 NS slot-products of a k-quarter are packed
// into four MFMAs (NS = 5) or three (NS <= 4) instead: ktup_split_plan.h says which piece of which logit group sits in which slot on both
// sides and proves, in static_asserts, that every product occurs exactly once.  The A planes are staged from that table (three per table
// at NS = 5, as before; two at NS <= 4), the B operands are conversions of fp32 vectors arranged by it from the lane's own logits and
// their residues -- nothing crosses lanes, and a pair stays one MFMA column.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "ktup_common.h"
#include "ktup_pref_geom.h"
#include "ktup_lane_swap.h"
#include "ktup_split_plan.h"

namespace ktup {
namespace {

// ---- split stage 2: an fp32 value as three bf16 pieces.  hi = bf16(x), mid = bf16(x - hi), lo = x - hi - mid (round to nearest each
// time): both differences are exact in fp32 and the last one has at most 8 significant bits, so hi + mid + lo == x.
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef float f8 __attribute__((ext_vector_type(8)));
struct Split3 { bf8 hi, mid, lo; };
KTUP_DEV Split3 split3(const f8 x) {
  Split3 r;
  r.hi = __builtin_convertvector(x, bf8);
  const f8 r1 = x - __builtin_convertvector(r.hi, f8);
  r.mid = __builtin_convertvector(r1, bf8);
  const f8 r2 = r1 - __builtin_convertvector(r.mid, f8);
  r.lo = __builtin_convertvector(r2, bf8);
  return r;
}
// table . logits over 32 preference slots with fp32-grade products: every bf16 x bf16 product is exact in the fp32 accumulator, and the
// six kept ones hold every term above 2^-24 of the full product (dropped: mid.lo, lo.mid, lo.lo); smallest terms first
KTUP_DEV v4 mfma_split(const bf8 ah, const bf8 am, const bf8 al, const Split3& b, v4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b.lo, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, b.hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, b.mid, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b.mid, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, b.hi, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b.hi, acc, 0, 0, 0);
}

// compile-time loop: f(std::integral_constant<int, 0>) .. f(std::integral_constant<int, N - 1>), so that a body can index the constexpr plan
template <int N, typename F>
KTUP_DEV void static_for(F&& f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}
// one piece of group `group` of a split vector, or zero, as the plan's term says
template <int PIECE, int GROUP>
KTUP_DEV __bf16 plan_piece(const Split3& v) {
  if constexpr (PIECE == split_plan::HI) return v.hi[GROUP];
  else if constexpr (PIECE == split_plan::MID) return v.mid[GROUP];
  else if constexpr (PIECE == split_plan::LO) return v.lo[GROUP];
  else return (__bf16)0.f;
}
// the B operand of MFMA M of the plan as an fp32 vector to convert: the hi piece of group s is bf16(x[s]), the mid piece bf16(r1[s]) with
// r1 = x - hi, the lo piece bf16(r2[s]) with r2 = r1 - mid
template <int NS, int M>
KTUP_DEV f8 plan_b_arranged(const float* x, const float* r1, const float* r2) {
  f8 v;
  static_for<8>([&](auto sl) {
    constexpr split_plan::Term t = split_plan::plan_for(NS).mfma[M].b[decltype(sl)::value];
    if constexpr (t.piece == split_plan::HI) v[decltype(sl)::value] = x[t.group];
    else if constexpr (t.piece == split_plan::MID) v[decltype(sl)::value] = r1[t.group];
    else if constexpr (t.piece == split_plan::LO) v[decltype(sl)::value] = r2[t.group];
    else v[decltype(sl)::value] = 0.f;
  });
  return v;
}
// table . logits by the plan: p0 = this lane's chunk of the tile's coordinate in plane 0 (planes PLQ chunks apart), pb = the B operands in
// issue order (smallest terms first)
template <int NS, int PLQ>
KTUP_DEV v4 mfma_packed(const bf8* p0, const bf8 (&pb)[4], v4 acc) {
  constexpr int NPL = split_plan::plan_for(NS).nplanes, NM = split_plan::plan_for(NS).nmfma;
  bf8 ap[NPL];
#pragma unroll
  for (int pl = 0; pl < NPL; ++pl) ap[pl] = p0[pl * PLQ];
  static_for<NM>([&](auto m) {
    constexpr int M = decltype(m)::value;
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[split_plan::plan_for(NS).mfma[M].plane], pb[M], acc, 0, 0, 0);
  });
  return acc;
}

enum { SPLIT_FP32 = 0, SPLIT_SIX = 1, SPLIT_PACK = 2 };   // stage 2 of the soft gate: fp32 MFMAs, six bf16 products, the packed plan

template <int NCH_, int NP_, bool HASE_, bool HARD_, int SPLIT_ = SPLIT_FP32>
struct McGeom {
  static constexpr int NCH = NCH_, NP = NP_;
  static constexpr bool HASE = HASE_, HARD = HARD_;   // HARD: straight-through Gumbel gate (forward value = one-hot)
  static constexpr bool SPLIT = SPLIT_ != SPLIT_FP32; // soft gate: stage 2 on v_mfma_f32_16x16x32_bf16, operands as three bf16 pieces
  static constexpr bool PACK = SPLIT_ == SPLIT_PACK;  //   ... with the products packed by ktup_split_plan.h (NS = NP logits per lane)
  static constexpr int NPL = PACK ? split_plan::plan_for(NP_).nplanes : 3;   // SPLIT: bf16 planes per table
  static_assert(!(SPLIT && HARD) && !(SPLIT && NP > 8), "the split stage 2 is the soft gate's, K = 32 preference slots");
  static_assert(!PACK || (NP >= 3 && NP <= 5 && split_plan::plan_for(NP_).ns == NP_), "the packed plans are for three to five logits per lane");
  static constexpr int D = 4 * NCH;
  static constexpr int KG = (D + 15) / 16;               // stage-1 k groups of 16 coordinates
  static constexpr int CT = KG;                          // stage-2 coordinate tiles of 16
  static constexpr int REM = NP * 4 - ((NP * 4 - 1) / 16) * 16;   // slots used in the last 16-slot tile (multiple of 4)
  static constexpr bool REM4 = (NP > 4) && REM == 4;     // last tile = one group of <= 4 preferences -> 4x4x1 path
  static constexpr int PT = (NP + 3) / 4;                // 16-slot preference tiles (including a REM4 tile)
  static constexpr int PTF = REM4 ? PT - 1 : PT;         // tiles computed with 16x16x4
  static constexpr bool TAIL1 = NCH - 4 * (KG - 1) == 1;  // the last k group / coordinate tile holds ONE float4 chunk (d = 100):
  static constexpr int KGF = TAIL1 ? KG - 1 : KG;        //   stage 1 finishes with one b32-operand MFMA instead of four,
  static constexpr bool TAIL2 = TAIL1 && !SPLIT;         //   stage 2 does those 4 coordinates with 4x4x1 MFMAs -- the split stage 2
  static constexpr int CTF = TAIL2 ? CT - 1 : CT;        //   takes them as one more 16-coordinate tile (6 x 16 clk against 2 NP x 8 + a scatter)
  static constexpr int J = (16 * NCH + 63) / 64;         // float4 loads per lane, table and tile
  static constexpr int TOTAL = 16 * NCH;
  static constexpr int PITCHA4 = 4 * KG + 1;             // odd float4 pitch of the slot-ordered logit table
  static constexpr int KQ = (NCH + 3) / 4;               // REM4: float4 chunks per k-quarter
  static constexpr int TROW = 4 * NP;
  static constexpr int TPITCH = 16 * CT + ((16 * CT) % 32 == 0 ? 16 : 0);   // == 16 (mod 32)
  static constexpr int A_F4 = PTF * 16 * PITCHA4;        // float4s of the 16x16x4 logit table
  static constexpr int A4_F4 = REM4 ? 4 * 4 * KQ : 0;    // REM4 table: [4 prefs][4 quarters][KQ] float4
  static constexpr int HP = NCH | 1;                     // HARD: odd float4 pitch of the row-major tables (one row is looked up per pair)
  static constexpr int PLANE_Q = 16 * CT * 4;            // SPLIT: 16-byte chunks of one bf16 plane, [16 CT coordinates][4 k-quarters] x 8 slots
  static constexpr int T_F = SPLIT ? NPL * PLANE_Q * 4 : HARD ? TROW * HP * 4 : TROW * TPITCH;   // floats per stage-2 table (SPLIT: NPL planes)
  static constexpr size_t TABLE_BYTES = (size_t)(A_F4 + A4_F4) * 16 + (size_t)2 * T_F * 4;
  static constexpr int XT_F4 = 16 * NCH + 3;             // x / q tile + 3 zero chunks (stage-1 reads run past the last row)
  static constexpr int NOISE_F = HARD ? 16 * TROW : 0;   // HARD: Gumbel noise of the tile, [pair][preference]
  static constexpr size_t WAVE_BYTES = ((size_t)XT_F4 * 16 + 3 * 16 * 4 + (size_t)NOISE_F * 4 + 15) & ~(size_t)15;
  static constexpr int NW_MAX = (int)((160 * 1024 - TABLE_BYTES) / WAVE_BYTES);
  static constexpr int NW = NW_MAX >= 16 ? 16 : NW_MAX >= 4 ? (NW_MAX & ~3) : NW_MAX;   // < 2: the geometry does not fit (d = 256 with P > 20)
};

struct McArgs {
  const v4 *U, *I, *E;
  uint32_t ldu4, ldi4, lde4;
  const int32_t* item2ent;
  const float *Alog, *Ar, *Cn;   // prepared tables, row pitch dp floats
  int dp, P, l1;
  int gumbel;                    // KTUP_GUMBEL_* (HARD kernels): INPUT reads `uniform` (n x P), PHILOX draws (seed, offset)
  const float* uniform;
  uint64_t seed, offset;
  const int64_t *u_ids, *i_ids;
  int64_t n;
  float* score;
  int nt;                        // row gathers with the nontemporal hint (option nt_gather: tables far beyond the Infinity Cache)
};

// L1: the distance is compile-time too -- with a run-time flag the compiler evaluates |z| AND z^2 for every coordinate and
// selects (v_and + v_cndmask per element: ~70 of a tile's ~330 VALU instructions).
//
// BUF (option fwd_buf_gather, soft gate, d <= 128): the 16 lanes that load a tile's ids also form each row's BYTE offset id * pitch, once,
// and the sid slots hold its low 32 bits instead of the id; the row loads are buffer loads (one descriptor per table in scalar
// registers: base = the table, 2^32 - 1 records) whose 32-bit lane offset is ONE v_add_u32 of the row's offset and the lane's
// loop-invariant chunk offset -- with 64-bit pointers every lane rebuilt id * pitch + chunk for every load (11 instructions on 64-bit
// pairs per load group of three tables).  The library's ABI carries no row counts, so the kernel decides per tile: a tile is FAST when
// every one of its 48 rows ends at or below byte 2^32 - 1 of its table (one ballot of the id lanes; the flag travels with the
// prefetched offsets); any other tile re-reads its ids and gathers through 64-bit pointers as the !BUF kernel does.
template <typename G, bool L1, bool BUF = false>
__global__ __launch_bounds__(G::NW * 64) void pref_fwd_mc_kernel(McArgs a) {
  static_assert(!BUF || (!G::HARD && G::NCH <= 32), "the buffer-load gather is the soft gate's, d <= 128");
  KTUP_RESOLVE_GUMBEL(a);
  constexpr int NCH = G::NCH, NP = G::NP, KG = G::KG, CT = G::CT, PTF = G::PTF, J = G::J, TOTAL = G::TOTAL;
  constexpr int PITCHA4 = G::PITCHA4, TPITCH = G::TPITCH, KQ = G::KQ;
  constexpr bool HASE = G::HASE, REM4 = G::REM4, TAIL1 = G::TAIL1, HARD = G::HARD, SPLIT = G::SPLIT, TAIL2 = G::TAIL2;
  constexpr int PLQ = G::PLANE_Q;
  constexpr int HP = G::HP;
  constexpr int KGF = G::KGF, CTF = G::CTF;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4* AlogS = reinterpret_cast<v4*>(smem);                       // [PTF * 16 slots][PITCHA4]
  v4* A4S = AlogS + G::A_F4;                                     // REM4: [4 prefs][4 quarters][KQ]
  float* CnS = reinterpret_cast<float*>(A4S + G::A4_F4);         // [TROW][TPITCH]
  float* ArS = CnS + G::T_F;
  const int t = threadIdx.x, lane = t & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nthr = blockDim.x, nwr = nthr >> 6;                  // waves actually launched (<= G::NW; fewer for small batches)
  char* wbase = reinterpret_cast<char*>(ArS + G::T_F) + (size_t)w * G::WAVE_BYTES;
  v4* xt = reinterpret_cast<v4*>(wbase);                         // [16 * NCH] + 3 zero chunks
  int32_t* sid = reinterpret_cast<int32_t*>(xt + G::XT_F4);      // [3][16]
  float* noise = reinterpret_cast<float*>(sid + 48);             // HARD: [16][TROW]
  // ---- stage the tables once per workgroup
  {
    // float4 granularity (table rows are 16-byte aligned with a pitch that is a multiple of 4 floats): for a B=512 step this
    // staging is a visible part of the launch
    const int P = a.P, dp = a.dp;
    const v4 zero = (v4){0.f, 0.f, 0.f, 0.f};
    for (int idx = t; idx < G::A_F4; idx += nthr) {
      const int srow = idx / PITCHA4, c = idx - srow * PITCHA4;
      const int tt = srow >> 4, i = srow & 15;
      const int p = 16 * tt + 4 * (i & 3) + (i >> 2);            // slot -> preference (block transposed)
      AlogS[idx] = (p < P && c < NCH) ? *reinterpret_cast<const v4*>(a.Alog + p * dp + 4 * c) : zero;
    }
    if (REM4) {
      for (int idx = t; idx < G::A4_F4; idx += nthr) {     // [pref i][quarter kp][KQ chunks]
        const int i = idx / (4 * KQ), rem = idx - i * (4 * KQ);
        const int kp = rem / KQ, kk = rem - kp * KQ;
        const int p = 16 * PTF + i, c = KQ * kp + kk;
        A4S[idx] = (p < P && c < NCH) ? *reinterpret_cast<const v4*>(a.Alog + p * dp + 4 * c) : zero;
      }
    }
    if constexpr (SPLIT) {
      // three bf16 planes per table, [coordinate c][k-quarter][8 slots]: lane (kq, j) of the 16x16x32 MFMA reads the A operand of
      // coordinate 16 ct + j as ONE 16-byte chunk.  Slot (kq, s) = preference 4 s + kq = 16 tt + 4 reg + kq with s = 4 tt + reg: the
      // preferences whose logits lg[tt][reg] lane (kq, .) holds after stage 1.  The chunks of coordinates with bit 3 set sit two places on
      // (kq ^ 2): a 16-lane group of ds_read_b128 is rows {0-3, 12-15} of one quarter + rows 4-11 of the next, and rows 8 apart
      // (64-byte rows) would share their banks.
      bf8* CnP = reinterpret_cast<bf8*>(CnS);
      bf8* ArP = reinterpret_cast<bf8*>(ArS);
      constexpr int NC = 16 * CT;
      for (int idx = t; idx < 4 * NC; idx += nthr) {
        const int kqs = idx / NC, c = idx - kqs * NC;
        f8 vn, vr;
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) {
          const int p = 4 * sl + kqs;
          const bool ok = p < P && c < 4 * NCH;
          vn[sl] = ok ? a.Cn[p * dp + c] : 0.f;
          vr[sl] = ok ? a.Ar[p * dp + c] : 0.f;
        }
        const Split3 sn = split3(vn), sr = split3(vr);
        const int o = 4 * c + (kqs ^ ((c >> 2) & 2));
        if constexpr (G::PACK) {
          // the plan's planes: slot sl of plane pl holds the piece the table names, of the group it names (groups >= NP are zero: P <= 4 NP)
          static_for<G::NPL>([&](auto pl) {
            bf8 cn, cr;
            static_for<8>([&](auto sl) {
              constexpr split_plan::Term tm = split_plan::plan_for(NP).plane[decltype(pl)::value][decltype(sl)::value];
              cn[decltype(sl)::value] = plan_piece<tm.piece, tm.group>(sn);
              cr[decltype(sl)::value] = plan_piece<tm.piece, tm.group>(sr);
            });
            CnP[decltype(pl)::value * PLQ + o] = cn;
            ArP[decltype(pl)::value * PLQ + o] = cr;
          });
        } else {
          CnP[o] = sn.hi; CnP[PLQ + o] = sn.mid; CnP[2 * PLQ + o] = sn.lo;
          ArP[o] = sr.hi; ArP[PLQ + o] = sr.mid; ArP[2 * PLQ + o] = sr.lo;
        }
      }
    } else {
      constexpr int pitch4 = HARD ? HP : TPITCH / 4;
      v4* Cn4 = reinterpret_cast<v4*>(CnS);
      v4* Ar4 = reinterpret_cast<v4*>(ArS);
      for (int idx = t; idx < G::T_F / 4; idx += nthr) {
        const int p = idx / pitch4, c = idx - p * pitch4;
        const bool ok = p < P && c < NCH;
        Cn4[idx] = ok ? *reinterpret_cast<const v4*>(a.Cn + p * dp + 4 * c) : zero;
        Ar4[idx] = ok ? *reinterpret_cast<const v4*>(a.Ar + p * dp + 4 * c) : zero;
      }
    }
    if (lane < 3) xt[16 * NCH + lane] = (v4){0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();
  // ---- loop-invariant lane geometry
  int grow[J], gc[J];                                            // (row, chunk) of this lane's jj-th load
#pragma unroll
  for (int jj = 0; jj < J; ++jj) {
    const int e = lane + 64 * jj;
    const bool past = e >= TOTAL;                                // lanes past the tile re-read chunk 0 of row 0 (never stored)
    grow[jj] = past ? 0 : e / NCH;
    gc[jj] = past ? 0 : e % NCH;
  }
  const bool last_ok = lane + 64 * (J - 1) < TOTAL;
  // BUF: the descriptors, the lane's chunk byte offsets, and what turns an id into its row's offset.  id * pitch in float4 units is exact
  // in 64 bits (two 32-bit factors); the row [16 o, 16 o + 16 NCH) ends at or below byte 2^32 - 1 iff o <= 2^28 - 1 - NCH.
  [[maybe_unused]] __amdgpu_buffer_rsrc_t rsU, rsI, rsE;
  [[maybe_unused]] uint32_t gcb[J];
  if constexpr (BUF) {
    rsU = __builtin_amdgcn_make_buffer_rsrc(const_cast<v4*>(a.U), 0, (int)0xffffffffu, 0x00020000);
    rsI = __builtin_amdgcn_make_buffer_rsrc(const_cast<v4*>(a.I), 0, (int)0xffffffffu, 0x00020000);
    rsE = __builtin_amdgcn_make_buffer_rsrc(const_cast<v4*>(HASE ? a.E : a.U), 0, (int)0xffffffffu, 0x00020000);
#pragma unroll
    for (int jj = 0; jj < J; ++jj) gcb[jj] = 16u * (uint32_t)gc[jj];
  }
  constexpr uint64_t OMAX = (1ull << 28) - 1 - NCH;
  bool fast = true;                                              // BUF: this tile's rows are all in reach of 32-bit offsets (wave-uniform)
  const v4* xb = xt + j * NCH + kq;                              // stage-1 B operand / q rows of this lane
  const v4* tab = AlogS + j * PITCHA4 + kq;                      // stage-1 A operand
  const float* tn0 = CnS + kq * TPITCH + j;
  const float* tr0 = ArS + kq * TPITCH + j;
  const bf8* pn0 = reinterpret_cast<const bf8*>(CnS) + 4 * j + (kq ^ ((j >> 2) & 2));   // SPLIT: this lane's chunk of coordinate j, plane hi
  const bf8* pr0 = reinterpret_cast<const bf8*>(ArS) + 4 * j + (kq ^ ((j >> 2) & 2));
  constexpr bool l1 = L1;
  const int64_t ntiles = (a.n + 15) / 16;
  const int64_t wstride = (int64_t)gridDim.x * nwr;
  bool first = true;
  for (int64_t tile_id = (int64_t)blockIdx.x * nwr + w; tile_id < ntiles; tile_id += wstride) {
    // wave-uniform 64-bit tile origin (scalar registers) + 32-bit lane offsets: kept as 64-bit per-lane row indices, these were
    // six registers the kernel had to spill at 128 -- with scratch reloads in front of the id loads and inside the matrix phases
    const int64_t row0 = tile_id * 16;
    const int rem = (int)(a.n - row0 < 16 ? a.n - row0 : 16);
    // SPLIT: the id loads index with a per-tile opaque copy of the lane number -- hoisted out of the tile loop, the 64-bit byte offset
    // of the lane is the register pair that tips this kernel over 128 (it was spilled, and reloaded in front of every id load)
    int idl = lane;
    if constexpr (SPLIT || BUF) asm volatile("" : "+v"(idl));
    bool far = false;
    if (first && lane < 16) {
      const bool ok = lane < rem;
      const int64_t uid = ok ? (a.u_ids + row0)[idl] : 0, iid = ok ? (a.i_ids + row0)[idl] : 0;
      if constexpr (BUF) {
        const uint64_t ou = (uint64_t)(uint32_t)uid * a.ldu4, oi = (uint64_t)(uint32_t)iid * a.ldi4;
        const uint64_t oe = HASE ? (uint64_t)(uint32_t)a.item2ent[iid] * a.lde4 : 0;
        far = ou > OMAX || oi > OMAX || oe > OMAX;
        sid[lane] = (int32_t)((uint32_t)ou << 4);
        sid[16 + lane] = (int32_t)((uint32_t)oi << 4);
        sid[32 + lane] = (int32_t)((uint32_t)oe << 4);
      } else {
        sid[lane] = (int32_t)uid;
        sid[16 + lane] = (int32_t)iid;
        sid[32 + lane] = HASE ? a.item2ent[iid] : 0;
      }
    }
    if constexpr (BUF) {
      if (first) fast = __builtin_amdgcn_ballot_w64(far) == 0;
    }
    first = false;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- gather: x -> LDS tile, q in registers.  Two batches of row loads: 16 waves x 3 x JA KB in flight per CU is
    // already several times the latency-bandwidth product, and 3 x J live float4 would push the kernel past 128 VGPRs.
    v4 q[J];
    constexpr int JA = G::NW >= 16 ? (J + 1) / 2 : J;
    if constexpr (BUF) {
      auto gather = [&](auto by_offset) {                        // by_offset: buffer loads at the 32-bit offsets in the sid slots
        constexpr bool OFFS = decltype(by_offset)::value;
#pragma unroll
        for (int j0 = 0; j0 < J; j0 += JA) {
          v4 uu[JA], vv[JA], ee[JA];
#pragma unroll
          for (int jb = 0; jb < JA; ++jb) {
            const int jj = j0 + jb;
            if (jj < J) {
              if constexpr (OFFS) {
                uu[jb] = __builtin_bit_cast(v4, __builtin_amdgcn_raw_buffer_load_b128(rsU, (int)((uint32_t)sid[grow[jj]] + gcb[jj]), 0, 0));
                vv[jb] = __builtin_bit_cast(v4, __builtin_amdgcn_raw_buffer_load_b128(rsI, (int)((uint32_t)sid[16 + grow[jj]] + gcb[jj]), 0, 0));
                if (HASE) ee[jb] = __builtin_bit_cast(v4, __builtin_amdgcn_raw_buffer_load_b128(rsE, (int)((uint32_t)sid[32 + grow[jj]] + gcb[jj]), 0, 0));
              } else {
                uint32_t gs = gcb[jj];
                asm volatile("" : "+v"(gs));   // opaque, as gc[jj] in the pointer kernel: nothing of this cold branch is worth a register outside it
                uu[jb] = a.U[(uint64_t)(uint32_t)sid[grow[jj]] * a.ldu4 + (gs >> 4)];
                vv[jb] = a.I[(uint64_t)(uint32_t)sid[16 + grow[jj]] * a.ldi4 + (gs >> 4)];
                if (HASE) ee[jb] = a.E[(uint64_t)(uint32_t)sid[32 + grow[jj]] * a.lde4 + (gs >> 4)];
              }
            }
          }
#pragma unroll
          for (int jb = 0; jb < JA; ++jb) {
            const int jj = j0 + jb;
            if (jj < J) {
              const v4 ve = HASE ? vv[jb] + ee[jb] : vv[jb];
              if (jj < J - 1 || last_ok) xt[lane + 64 * jj] = uu[jb] + ve;
              q[jj] = uu[jb] + (-ve);
            }
          }
        }
      };
      if (__builtin_expect(fast, 1)) {
        gather(std::true_type{});
      } else {
        // cold: a row of this tile lies (partly) past byte 2^32 - 1 of its table.  Its ids once more, into the sid slots in place of
        // the offsets, and the gather through 64-bit pointers
        if (lane < 16) {
          const bool ok = lane < rem;
          const int64_t uid = ok ? (a.u_ids + row0)[idl] : 0, iid = ok ? (a.i_ids + row0)[idl] : 0;
          sid[lane] = (int32_t)uid;
          sid[16 + lane] = (int32_t)iid;
          sid[32 + lane] = HASE ? a.item2ent[iid] : 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        gather(std::false_type{});
      }
    } else {
#pragma unroll
    for (int j0 = 0; j0 < J; j0 += JA) {
      v4 uu[JA], vv[JA], ee[JA];
#pragma unroll
      for (int jb = 0; jb < JA; ++jb) {
        const int jj = j0 + jb;
        if (jj < J) {
          asm volatile("" : "+v"(gc[jj]));   // opaque per tile: LICM would hoist 3 x J 64-bit (table + chunk) bases and spill them
          const uint32_t idu = (uint32_t)sid[grow[jj]], idi = (uint32_t)sid[16 + grow[jj]];
          const v4* pu = a.U + ((uint64_t)idu * a.ldu4 + (uint32_t)gc[jj]);
          const v4* pv = a.I + ((uint64_t)idi * a.ldi4 + (uint32_t)gc[jj]);
          // scattered rows of tables much larger than the caches: the default policy allocates every line it will never
          // re-read (tools/gather_bench footprint: 4.68 vs 4.86 TB/s at 9.7 GB; the other way round below ~2 GB)
          uu[jb] = a.nt ? __builtin_nontemporal_load(pu) : *pu;
          vv[jb] = a.nt ? __builtin_nontemporal_load(pv) : *pv;
          if (HASE) {
            const uint32_t ide = (uint32_t)sid[32 + grow[jj]];
            const v4* pe = a.E + ((uint64_t)ide * a.lde4 + (uint32_t)gc[jj]);
            ee[jb] = a.nt ? __builtin_nontemporal_load(pe) : *pe;
          }
        }
      }
#pragma unroll
      for (int jb = 0; jb < JA; ++jb) {
        const int jj = j0 + jb;
        if (jj < J) {
          const v4 ve = HASE ? vv[jb] + ee[jb] : vv[jb];
          if (jj < J - 1 || last_ok) xt[lane + 64 * jj] = uu[jb] + ve;
          q[jj] = uu[jb] + (-ve);
        }
      }
    }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- next tile's ids travel under the matrix phases
    int32_t nx_u = 0, nx_i = 0, nx_e = 0;
    bool nx_far = false;
    const bool pre = lane < 16 && tile_id + wstride < ntiles;
    if (pre) {
      const int64_t row1 = (tile_id + wstride) * 16;
      const bool ok = lane < a.n - row1;
      const int64_t uid = ok ? (a.u_ids + row1)[idl] : 0, iid = ok ? (a.i_ids + row1)[idl] : 0;
      if constexpr (BUF) {
        const uint64_t ou = (uint64_t)(uint32_t)uid * a.ldu4, oi = (uint64_t)(uint32_t)iid * a.ldi4;
        const uint64_t oe = HASE ? (uint64_t)(uint32_t)a.item2ent[iid] * a.lde4 : 0;
        nx_far = ou > OMAX || oi > OMAX || oe > OMAX;
        nx_u = (int32_t)((uint32_t)ou << 4); nx_i = (int32_t)((uint32_t)oi << 4); nx_e = (int32_t)((uint32_t)oe << 4);
      } else {
        nx_u = (int32_t)uid; nx_i = (int32_t)iid;
        nx_e = HASE ? a.item2ent[iid] : 0;
      }
    }
    // ---- stage 1: logits^T.  lg[tt][reg] of lane (kq, pair j) = logit of preference 16 tt + 4 reg + kq
    v4 lg[G::PT];
#pragma unroll
    for (int tt = 0; tt < G::PT; ++tt) lg[tt] = (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int gk = 0; gk < KGF; ++gk) {
      v4 bv = xb[4 * gk];
      if (4 * gk + 3 >= NCH) {                                   // chunks past the row (table is zero there): see REM4 note
        if (4 * gk + kq >= NCH) bv = (v4){0.f, 0.f, 0.f, 0.f};
      }
      v4 av[PTF];
#pragma unroll
      for (int tt = 0; tt < PTF; ++tt) av[tt] = tab[tt * 16 * PITCHA4 + 4 * gk];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int tt = 0; tt < PTF; ++tt) lg[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tt][c], bv[c], lg[tt], 0, 0, 0);
      }
    }
    if (TAIL1) {                                                 // coordinates 16 KGF + kq: one MFMA, scalar operands
      const float bs = reinterpret_cast<const float*>(xt + j * NCH + 4 * KGF)[kq];
#pragma unroll
      for (int tt = 0; tt < PTF; ++tt) {
        const float as = reinterpret_cast<const float*>(AlogS + (tt * 16 + j) * PITCHA4 + 4 * KGF)[kq];
        lg[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bs, lg[tt], 0, 0, 0);
      }
    }
    if (REM4) {
      // 16 blocks of 4x4x1: block b = lane >> 2 = (k-quarter kp = b >> 2 == kq, pair group pg = b & 3), A row i = lane & 3
      // = preference 16 PTF + i, B column jb = lane & 3 = pair 4 pg + jb.  D[reg i] of lane (b, jb) sums over the quarter.
      const int pg = (lane >> 2) & 3, jb = lane & 3;
      const v4* a4 = A4S + (jb * 4 + kq) * KQ;                   // row (pref jb, quarter kq)
      const v4* b4 = xt + (4 * pg + jb) * NCH + kq * KQ;         // pair 4 pg + jb, quarter kq
      v4 acc = (v4){0.f, 0.f, 0.f, 0.f}, acc1 = acc;              // two chains: a 4x4x1 result is not ready for the next issue slot
#pragma unroll
      for (int kk = 0; kk < KQ; ++kk) {
        const v4 av = a4[kk];
        v4 bv = b4[kk];
        if (3 * KQ + kk >= NCH) {                                // the last quarter runs past the row: A is zero there,
          if (kq * KQ + kk >= NCH) bv = (v4){0.f, 0.f, 0.f, 0.f};   // but keep a neighbour's inf / nan out of 0 * x
        }
#pragma unroll
        for (int c = 0; c < 4; c += 2) {
          acc = __builtin_amdgcn_mfma_f32_4x4x1f32(av[c], bv[c], acc, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(av[c + 1], bv[c + 1], acc1, 0, 0, 0);
        }
      }
      acc += acc1;
      // lane (kq, pair j16 = lane & 15) needs preference 16 PTF + kq of pair j16 = 4 pg + jb, summed over the 4 k-quarters
      // held by lanes l, l^16, l^32, l^48 (same block position): a reduce-scatter over kq
      const float mine = scatter_kq(acc);
      lg[PTF] = (v4){mine, 0.f, 0.f, 0.f};
    }
    // ---- q overwrites x
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
      if (jj < J - 1 || last_ok) xt[lane + 64 * jj] = q[jj];
    }
    v4 dacc = (v4){0.f, 0.f, 0.f, 0.f};
    if constexpr (HARD) {
      // ---- ST-Gumbel gate (transUP.py:118-170): y = one_hot(argmax_p(logit_p + g_p)), g = -log(-log(u + eps) + eps); the
      // forward value of the straight-through estimator is exactly the one-hot, so r = Ar[p*], n = Cn[p*].
      const int64_t grow = min(row0 + j, a.n - 1);
      const uint64_t base = (uint64_t)grow * (uint64_t)a.P;
      float best = -INFINITY;
      int bp = 0x7fffffff;
      if (a.gumbel == KTUP_GUMBEL_PHILOX) {
        // same stream as the other kernels (ktup_score_pref.hip draw_uniform): word (idx & 3) of Philox block idx >> 2,
        // idx = grow * P + p + offset.  The 4 kq lanes of a pair share its <= P/4 + 1 blocks and trade through LDS.
        const uint64_t i0 = base + a.offset, fb = i0 >> 2, lb = (i0 + (uint64_t)a.P - 1) >> 2;
        const Philox ph(a.seed);
        for (uint64_t b = fb + kq; b <= lb; b += 4) {
          const uint4 r = ph(b, 0x4b545550ull /* "KTUP" stream tag */);
          const uint32_t wds[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
          for (int wd = 0; wd < 4; ++wd) {
            const int64_t pp = (int64_t)((b << 2) + wd) - (int64_t)i0;
            if (pp >= 0 && pp < a.P) noise[j * G::TROW + (int)pp] = gumbel_from_uniform(u01(wds[wd]));
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int sidx = 0; sidx < NP; ++sidx) {                    // ascending p: strict > keeps the first maximum (torch.max)
        const int pp = 4 * sidx + kq;
        if (pp < a.P) {
          const float g = a.gumbel == KTUP_GUMBEL_PHILOX ? noise[j * G::TROW + pp] : gumbel_from_uniform(a.uniform[base + pp]);
          const float v = lg[sidx >> 2][sidx & 3] + g;
          if (v > best || bp == 0x7fffffff) { best = v; bp = pp; }
        }
      }
      // first-max over the 4 kq lanes: (value, preference) pairs, lower preference wins ties
      {
        const u2 rv = __builtin_amdgcn_permlane32_swap(__float_as_uint(best), __float_as_uint(best), false, false);
        const u2 rp = __builtin_amdgcn_permlane32_swap((unsigned)bp, (unsigned)bp, false, false);
        const float v0 = __uint_as_float(rv[0]), v1 = __uint_as_float(rv[1]);
        const int p0 = (int)rp[0], p1 = (int)rp[1];
        const bool take1 = p0 == 0x7fffffff || (p1 != 0x7fffffff && (v1 > v0 || (v1 == v0 && p1 < p0)));
        best = take1 ? v1 : v0; bp = take1 ? p1 : p0;
      }
      {
        const u2 rv = __builtin_amdgcn_permlane16_swap(__float_as_uint(best), __float_as_uint(best), false, false);
        const u2 rp = __builtin_amdgcn_permlane16_swap((unsigned)bp, (unsigned)bp, false, false);
        const float v0 = __uint_as_float(rv[0]), v1 = __uint_as_float(rv[1]);
        const int p0 = (int)rp[0], p1 = (int)rp[1];
        const bool take1 = p0 == 0x7fffffff || (p1 != 0x7fffffff && (v1 > v0 || (v1 == v0 && p1 < p0)));
        bp = take1 ? p1 : p0;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // q tile written above
      __builtin_amdgcn_wave_barrier();
      const v4* nrow = reinterpret_cast<const v4*>(CnS) + bp * HP + kq;
      const v4* rrow = reinterpret_cast<const v4*>(ArS) + bp * HP + kq;
      v4 sacc = (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {                          // lane (kq, j) owns q chunks 4 ct + kq
        if (4 * ct + 3 < NCH) {
          sacc += xb[4 * ct] * nrow[4 * ct];
        } else if (4 * ct < NCH) {
          if (4 * ct + kq < NCH) sacc += xb[4 * ct] * nrow[4 * ct];
        }
      }
      const float sfull = allsum_kq((sacc[0] + sacc[1]) + (sacc[2] + sacc[3]));
      const v4 ms = (v4){-sfull, -sfull, -sfull, -sfull};
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        bool on = 4 * ct + 3 < NCH;
        if (!on && 4 * ct < NCH) on = 4 * ct + kq < NCH;
        if (4 * ct < NCH) {
          if (on) {
            const v4 tv = __builtin_elementwise_fma(ms, nrow[4 * ct], xb[4 * ct] + rrow[4 * ct]);
            if (l1) dacc += __builtin_elementwise_abs(tv);
            else dacc = __builtin_elementwise_fma(tv, tv, dacc);
          }
        }
      }
    } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- stage 2a: n^T coordinate tiles
    v4 accN[CTF];
    Split3 lgs;                                                  // SPLIT: B[k = 8 kq + s][pair j] = the logit registers in hand, in pieces
    bf8 pb[4];                                                   // PACK: the plan's B operands, in issue order
    if constexpr (G::PACK) {
      // the last MFMA's operand holds the hi pieces and the one before it the mid pieces, group s in slot s (ktup_split_plan.h,
      // levels_in_place): the residues come from them, and every operand is ONE conversion of an fp32 vector arranged by the plan
      constexpr int NM = split_plan::plan_for(NP).nmfma;
      float x[NP], r1[NP], r2[NP];
#pragma unroll
      for (int s = 0; s < NP; ++s) x[s] = lg[s >> 2][s & 3];
      pb[NM - 1] = __builtin_convertvector(plan_b_arranged<NP, NM - 1>(x, r1, r2), bf8);
      const f8 hf = __builtin_convertvector(pb[NM - 1], f8);
#pragma unroll
      for (int s = 0; s < NP; ++s) r1[s] = x[s] - hf[s];
      pb[NM - 2] = __builtin_convertvector(plan_b_arranged<NP, NM - 2>(x, r1, r2), bf8);
      const f8 mf = __builtin_convertvector(pb[NM - 2], f8);
#pragma unroll
      for (int s = 0; s < NP; ++s) r2[s] = r1[s] - mf[s];
      static_for<NM - 2>([&](auto m) { pb[decltype(m)::value] = __builtin_convertvector(plan_b_arranged<NP, decltype(m)::value>(x, r1, r2), bf8); });
#pragma unroll
      for (int ct = 0; ct < CTF; ++ct) accN[ct] = mfma_packed<NP, PLQ>(pn0 + 64 * ct, pb, (v4){0.f, 0.f, 0.f, 0.f});
    } else if constexpr (SPLIT) {
      f8 g;
#pragma unroll
      for (int sl = 0; sl < 8; ++sl) g[sl] = (sl >> 2) < G::PT ? lg[(sl >> 2) < G::PT ? sl >> 2 : 0][sl & 3] : 0.f;
      lgs = split3(g);
#pragma unroll
      for (int ct = 0; ct < CTF; ++ct)
        accN[ct] = mfma_split(pn0[64 * ct], pn0[PLQ + 64 * ct], pn0[2 * PLQ + 64 * ct], lgs, (v4){0.f, 0.f, 0.f, 0.f});
    } else {
#pragma unroll
    for (int ct = 0; ct < CTF; ++ct) {
      accN[ct] = (v4){0.f, 0.f, 0.f, 0.f};
      float ta[NP];
#pragma unroll
      for (int m = 0; m < NP; ++m) ta[m] = tn0[(16 * (m >> 2) + 4 * (m & 3)) * TPITCH + 16 * ct];
#pragma unroll
      for (int m = 0; m < NP; ++m) accN[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(ta[m], lg[m >> 2][m & 3], accN[ct], 0, 0, 0);
    }
    }
    // TAIL1: the last 4 coordinates c0 + i (c0 = 16 CTF) on 4x4x1 blocks.  Block (kq, pair group): A row i = T[kq + 4 s][c0 + i],
    // B column = logit(kq + 4 s, pair) = lg[s >> 2][s & 3] of THIS lane, k step s.  n4 / r4 of lane (kq, pair) are partial
    // over the NP preferences {kq + 4 s}; the sum over kq comes with the s reduction (linear) or a reduce-scatter (distance).
    v4 n4 = (v4){0.f, 0.f, 0.f, 0.f}, r4 = n4, q4 = n4;
    if (TAIL2) {
      const float* tn4 = CnS + kq * TPITCH + 16 * CTF + (lane & 3);
      const float* tr4 = ArS + kq * TPITCH + 16 * CTF + (lane & 3);
      float tan[NP], tar[NP];
#pragma unroll
      for (int sidx = 0; sidx < NP; ++sidx) { tan[sidx] = tn4[4 * sidx * TPITCH]; tar[sidx] = tr4[4 * sidx * TPITCH]; }
#pragma unroll
      for (int sidx = 0; sidx < NP; ++sidx) {
        n4 = __builtin_amdgcn_mfma_f32_4x4x1f32(tan[sidx], lg[sidx >> 2][sidx & 3], n4, 0, 0, 0);
        r4 = __builtin_amdgcn_mfma_f32_4x4x1f32(tar[sidx], lg[sidx >> 2][sidx & 3], r4, 0, 0, 0);
      }
      q4 = xt[j * NCH + 4 * CTF];                                // q chunk of coordinates c0 .. c0 + 3 (same for the 4 kq lanes)
    }
    // ---- s = q . n   (lane (kq, j) owns coordinates 16 ct + 4 kq .. + 3 = q chunk 4 ct + kq of pair j)
    v4 sacc = TAIL2 ? q4 * n4 : (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < CTF; ++ct) {
      if (4 * ct + 3 < NCH) {
        sacc += xb[4 * ct] * accN[ct];
      } else if (4 * ct < NCH) {
        if (4 * ct + kq < NCH) sacc += xb[4 * ct] * accN[ct];
      }
    }
    const float sfull = allsum_kq((sacc[0] + sacc[1]) + (sacc[2] + sacc[3]));
    const v4 ms = (v4){-sfull, -sfull, -sfull, -sfull};
    // ---- stage 2b: r^T tiles and the distance
#pragma unroll
    for (int ct = 0; ct < CTF; ++ct) {
      float ta[NP];
      if constexpr (!SPLIT) {
#pragma unroll
        for (int m = 0; m < NP; ++m) ta[m] = tr0[(16 * (m >> 2) + 4 * (m & 3)) * TPITCH + 16 * ct];
      }
      v4 qv = (v4){0.f, 0.f, 0.f, 0.f};
      if (4 * ct + 3 < NCH) {
        qv = xb[4 * ct];
      } else if (4 * ct < NCH) {
        if (4 * ct + kq < NCH) qv = xb[4 * ct];
      }
      v4 accR = qv;                                              // q + r: start the accumulator at q
      if constexpr (G::PACK) {
        accR = mfma_packed<NP, PLQ>(pr0 + 64 * ct, pb, accR);
      } else if constexpr (SPLIT) {
        accR = mfma_split(pr0[64 * ct], pr0[PLQ + 64 * ct], pr0[2 * PLQ + 64 * ct], lgs, accR);
      } else {
#pragma unroll
        for (int m = 0; m < NP; ++m) accR = __builtin_amdgcn_mfma_f32_16x16x4f32(ta[m], lg[m >> 2][m & 3], accR, 0, 0, 0);
      }
      const v4 tv = __builtin_elementwise_fma(ms, accN[ct], accR);
      if (l1) dacc += __builtin_elementwise_abs(tv);
      else dacc = __builtin_elementwise_fma(tv, tv, dacc);
    }
    if (TAIL2) {                                                 // lane kq takes coordinate c0 + kq
      const float nf = scatter_kq(n4), rf = scatter_kq(r4);
      const float qe = kq == 0 ? q4[0] : kq == 1 ? q4[1] : kq == 2 ? q4[2] : q4[3];
      const float tv = fmaf(-sfull, nf, qe + rf);
      dacc[0] += l1 ? fabsf(tv) : tv * tv;
    }
    }
    const float score = allsum_kq((dacc[0] + dacc[1]) + (dacc[2] + dacc[3]));
    if (kq == 0 && j < rem) (a.score + row0)[j] = score;
    if (pre) { sid[lane] = nx_u; sid[16 + lane] = nx_i; sid[32 + lane] = nx_e; }
    if constexpr (BUF) fast = __builtin_amdgcn_ballot_w64(nx_far) == 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- d = 256 (config 5's width), soft gate, large batches: FOUR waves share a 16-pair tile, 64 coordinates each ----------------
// The kernel above keeps a whole 16 x 256 tile per wave: 48 row loads of 16 bytes in flight per lane and the q tile in registers are
// 256 VGPRs + 42 AGPRs, its x tiles fill the LDS at four waves per CU -- ONE wave per SIMD, which gathers, then computes, then
// gathers: on HBM-resident tables 0.59 ms per 716,800 pairs = 0.47 of the HBM peak where the pure gather of the same 1 KB rows
// reaches 0.73-0.79 (profiles/r04_gather_footprint.txt).  Here a wave owns 64 coordinates of the tile (the split of
// ktup_score_pref_bwd_wide.hip): 12 row loads per lane, all of them for the NEXT tile and in flight under the current tile's matrix
// phases; 12 waves per CU (three tiles in flight, three waves per SIMD).  The price: the three contractions over d -- logits, s = q.n,
// the distance -- are per-wave partials summed across the four waves through LDS (three workgroup barriers per tile, partials
// always added in wave order).
template <int NP_, bool HASE_>
struct FwGeom {
  static constexpr int NP = NP_;                           // groups of four preferences: P <= 4 NP, NP in {4, 5}
  static constexpr bool HASE = HASE_;
  static constexpr int NCH = 64, NWC = 4, NCW = 16;        // float4 chunks per row; waves per tile; chunks per wave
  static constexpr int PITCHA4 = 4 * 16 + 1;               // the slot-ordered logit table of McGeom (odd float4 pitch)
  static constexpr int XP = NCW + 1;                       // odd float4 pitch of a wave's x / q tile
  static constexpr int TROW = 4 * NP, TPITCH = 16 * 16 + 16;
  static constexpr int A0_F4 = 16 * PITCHA4;               // preferences 0..15 (slot i = preference 4 (i & 3) + (i >> 2))
  static constexpr int A1_F4 = NP > 4 ? 4 * PITCHA4 : 0;   // preferences 16..19, row-major: their logits come from 4x4x1 blocks (a 16x16x4 tile
                                                           // would be fifteen sixteenths padding: 512 of a wave's 2,300 matrix clocks per tile)
  static constexpr int T_F = TROW * TPITCH;
  static constexpr size_t TABLE_BYTES = (size_t)(A0_F4 + A1_F4) * 16 + (size_t)2 * T_F * 4;
  static constexpr int NLG = NP > 4 ? 5 : 4;               // live logit registers per lane (the second tile's only live one is reg 0)
  static constexpr size_t WAVE_BYTES = (size_t)16 * XP * 16 + 48 * 4;
  static constexpr size_t GROUP_BYTES = NWC * WAVE_BYTES + (size_t)NWC * NLG * 64 * 4 + (size_t)2 * NWC * 16 * 4;
  static constexpr int TG_FIT = (int)((160 * 1024 - TABLE_BYTES) / GROUP_BYTES);
  static constexpr int TG = TG_FIT >= 3 ? 3 : TG_FIT;      // tile groups (of four waves) per workgroup: three -- with four (128 VGPRs per lane) the KTUP variants spill 13-24 registers
};

template <typename G, bool L1>
__global__ __launch_bounds__(768) void pref_fwd_wide_kernel(McArgs a) {
  constexpr int NP = G::NP, NCH = G::NCH, NWC = G::NWC, XP = G::XP, PITCHA4 = G::PITCHA4, TPITCH = G::TPITCH, NLG = G::NLG;
  constexpr bool HASE = G::HASE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4* A0S = reinterpret_cast<v4*>(smem);
  v4* A1S = A0S + G::A0_F4;                                      // [4][PITCHA4]
  float* CnS = reinterpret_cast<float*>(A1S + G::A1_F4);         // [TROW][TPITCH]
  float* ArS = CnS + G::T_F;
  const int t = threadIdx.x, lane = t & 63, kq = lane >> 4, j = lane & 15;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int grp = wv >> 2, w = wv & 3;                           // tile group; coordinate slice [64 w, 64 w + 64)
  const int nthr = blockDim.x, ngrp = nthr >> 8;
  char* gbase = reinterpret_cast<char*>(ArS + G::T_F) + (size_t)grp * G::GROUP_BYTES;
  v4* xt = reinterpret_cast<v4*>(gbase + (size_t)w * G::WAVE_BYTES);   // [16 pairs][XP]: this wave's 16 chunks of x, later of q
  int32_t* sid = reinterpret_cast<int32_t*>(xt + 16 * XP);       // [3][16]: ids of the tile whose rows are fetched next
  float* red = reinterpret_cast<float*>(gbase + NWC * G::WAVE_BYTES);  // [NWC][NLG][64] logit partials
  float* sred = red + NWC * NLG * 64;                            // [NWC][16]  q . n partials
  float* dred = sred + NWC * 16;                                 // [NWC][16]  distance partials
  {
    const int P = a.P, dp = a.dp;
    const v4 zero = (v4){0.f, 0.f, 0.f, 0.f};
    for (int idx = t; idx < G::A0_F4; idx += nthr) {
      const int i = idx / PITCHA4, c = idx - i * PITCHA4;
      const int p = 4 * (i & 3) + (i >> 2);
      A0S[idx] = (p < P && c < NCH) ? *reinterpret_cast<const v4*>(a.Alog + p * dp + 4 * c) : zero;
    }
    for (int idx = t; idx < G::A1_F4; idx += nthr) {
      const int r = idx / PITCHA4, c = idx - r * PITCHA4;
      A1S[idx] = (16 + r < P && c < NCH) ? *reinterpret_cast<const v4*>(a.Alog + (16 + r) * dp + 4 * c) : zero;
    }
    v4* Cn4 = reinterpret_cast<v4*>(CnS);
    v4* Ar4 = reinterpret_cast<v4*>(ArS);
    for (int idx = t; idx < G::T_F / 4; idx += nthr) {
      const int p = idx / (TPITCH / 4), c = idx - p * (TPITCH / 4);
      const bool ok = p < P && c < NCH;
      Cn4[idx] = ok ? *reinterpret_cast<const v4*>(a.Cn + p * dp + 4 * c) : zero;
      Ar4[idx] = ok ? *reinterpret_cast<const v4*>(a.Ar + p * dp + 4 * c) : zero;
    }
  }
  __syncthreads();
  const uint32_t gc = 16u * (uint32_t)w + (uint32_t)j;           // this lane's chunk of every row it fetches (rows kq, kq + 4, ..)
  const v4* xb = xt + j * XP + kq;                               // MFMA operand view: chunk 4 g + kq of pair j
  const v4* tab0 = A0S + j * PITCHA4 + kq + 16 * w;
  // preferences 16..19 on v_mfma_f32_4x4x1 (16 blocks): block (quarter kq of this wave's coordinates, pair group) -- lane (kq, pair j)
  // supplies A = preference 16 + (j & 3) and B = pair j at chunks 4 kq .. 4 kq + 3 of the slice
  const v4* tab1 = A1S + (j & 3) * PITCHA4 + 4 * kq + 16 * w;
  const v4* xb4 = xt + j * XP + 4 * kq;
  const float* tn0 = CnS + kq * TPITCH + j + 64 * w;
  const float* tr0 = ArS + kq * TPITCH + j + 64 * w;
  const int64_t ntiles = (a.n + 15) / 16;
  const int64_t tstride = (int64_t)gridDim.x * ngrp;
  const int64_t tfirst = (int64_t)blockIdx.x * ngrp;             // < ntiles (grid sizing)
  const int niter = (int)((ntiles - tfirst + tstride - 1) / tstride);   // the same for every wave of the workgroup (barriers)
  int32_t nx_u = 0, nx_i = 0, nx_e = 0;
  auto fetch_ids = [&](int64_t tile) {
    nx_u = 0; nx_i = 0; nx_e = 0;
    if (lane < 16 && tile < ntiles) {
      const int64_t row = tile * 16 + lane;
      const bool ok = row < a.n;
      const int64_t uid = ok ? a.u_ids[row] : 0, iid = ok ? a.i_ids[row] : 0;
      nx_u = (int32_t)uid; nx_i = (int32_t)iid;
      nx_e = HASE ? a.item2ent[iid] : 0;
    }
  };
  v4 uu[4], vv[4], ee[4];
  auto issue_rows = [&]() {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int row = kq + 4 * jj;
      const uint32_t idu = (uint32_t)sid[row], idi = (uint32_t)sid[16 + row];
      const v4* pu = a.U + ((uint64_t)idu * a.ldu4 + gc);
      const v4* pv = a.I + ((uint64_t)idi * a.ldi4 + gc);
      uu[jj] = a.nt ? __builtin_nontemporal_load(pu) : *pu;
      vv[jj] = a.nt ? __builtin_nontemporal_load(pv) : *pv;
      if (HASE) {
        const uint32_t ide = (uint32_t)sid[32 + row];
        const v4* pe = a.E + ((uint64_t)ide * a.lde4 + gc);
        ee[jj] = a.nt ? __builtin_nontemporal_load(pe) : *pe;
      }
    }
  };
  // ---- prologue: ids and rows of the first tile, ids of the second
  fetch_ids(tfirst + grp);
  if (lane < 16) { sid[lane] = nx_u; sid[16 + lane] = nx_i; sid[32 + lane] = nx_e; }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (tfirst + grp < ntiles) issue_rows();
  fetch_ids(tfirst + grp + tstride);
  for (int it = 0; it < niter; ++it) {
    const int64_t tile_id = tfirst + grp + (int64_t)it * tstride;
    const bool live = tile_id < ntiles;                          // wave-uniform
    v4 q[4];
    v4 lg0 = (v4){0.f, 0.f, 0.f, 0.f};
    if (live) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const v4 ve = HASE ? vv[jj] + ee[jj] : vv[jj];
        xt[(kq + 4 * jj) * XP + j] = uu[jj] + ve;
        q[jj] = uu[jj] + (-ve);
      }
    }
    if (lane < 16) { sid[lane] = nx_u; sid[16 + lane] = nx_i; sid[32 + lane] = nx_e; }   // (the rows of THIS tile were addressed before)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- the next tile's rows travel under this tile's phases, the ids of the tile after it too
    if (tile_id + tstride < ntiles) issue_rows();
    fetch_ids(tile_id + 2 * tstride);
    if (live) {
      // ---- stage 1: this wave's 64 coordinates of logits^T (layout of the kernel above: lg[reg] of lane (kq, pair j) = preference 4 reg + kq)
#pragma unroll
      for (int gk = 0; gk < 4; ++gk) {
        const v4 bv = xb[4 * gk];
        const v4 av0 = tab0[4 * gk];
#pragma unroll
        for (int c = 0; c < 4; ++c) lg0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[c], bv[c], lg0, 0, 0, 0);
      }
      float* rw = red + w * NLG * 64 + lane;
      rw[0] = lg0[0]; rw[64] = lg0[1]; rw[128] = lg0[2]; rw[192] = lg0[3];
      if (NP > 4) {
        v4 acc = (v4){0.f, 0.f, 0.f, 0.f}, acc1 = acc;               // two chains: a 4x4x1 result is not ready for the next issue slot
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const v4 av = tab1[kk], bv = xb4[kk];
          acc = __builtin_amdgcn_mfma_f32_4x4x1f32(av[0], bv[0], acc, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(av[1], bv[1], acc1, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_4x4x1f32(av[2], bv[2], acc, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(av[3], bv[3], acc1, 0, 0, 0);
        }
        acc += acc1;
        rw[256] = scatter_kq(acc);                                  // lane (kq, pair j): preference 16 + kq, summed over the four quarters
      }
      // ---- q overwrites x (this wave's own slice: its stage-1 reads are behind it)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) xt[(kq + 4 * jj) * XP + j] = q[jj];
    }
    __syncthreads();
    // the PREVIOUS tile's score: its distance partials were written before this barrier and are rewritten after the next one (a third
    // barrier per tile only for this store cost 2-3 % of the kernel)
    if (it > 0 && w == 0 && kq == 0) {
      const int64_t row0 = (tile_id - tstride) * 16;
      if (row0 + j < a.n) (a.score + row0)[j] = (dred[j] + dred[16 + j]) + (dred[32 + j] + dred[48 + j]);
    }
    v4 accN[4];
    float lgs[NLG];
    if (live) {
#pragma unroll
      for (int k = 0; k < NLG; ++k) {
        const float* r0 = red + k * 64 + lane;
        lgs[k] = (r0[0] + r0[NLG * 64]) + (r0[2 * NLG * 64] + r0[3 * NLG * 64]);
      }
      // ---- stage 2a: n^T for this wave's coordinates, s partial
      v4 sacc = (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        accN[ct] = (v4){0.f, 0.f, 0.f, 0.f};
        float ta[NP];
#pragma unroll
        for (int m = 0; m < NP; ++m) ta[m] = tn0[(16 * (m >> 2) + 4 * (m & 3)) * TPITCH + 16 * ct];
#pragma unroll
        for (int m = 0; m < NP; ++m) accN[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(ta[m], lgs[m], accN[ct], 0, 0, 0);
        sacc += xb[4 * ct] * accN[ct];
      }
      const float sp = allsum_kq((sacc[0] + sacc[1]) + (sacc[2] + sacc[3]));
      if (kq == 0) sred[w * 16 + j] = sp;
    }
    __syncthreads();
    if (live) {
      const float sfull = (sred[j] + sred[16 + j]) + (sred[32 + j] + sred[48 + j]);
      const v4 ms = (v4){-sfull, -sfull, -sfull, -sfull};
      v4 dacc = (v4){0.f, 0.f, 0.f, 0.f};
      // ---- stage 2b: r^T tiles and the distance
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        float ta[NP];
#pragma unroll
        for (int m = 0; m < NP; ++m) ta[m] = tr0[(16 * (m >> 2) + 4 * (m & 3)) * TPITCH + 16 * ct];
        v4 accR = xb[4 * ct];                                     // q + r: start the accumulator at q
#pragma unroll
        for (int m = 0; m < NP; ++m) accR = __builtin_amdgcn_mfma_f32_16x16x4f32(ta[m], lgs[m], accR, 0, 0, 0);
        const v4 tv = __builtin_elementwise_fma(ms, accN[ct], accR);
        if (L1) dacc += __builtin_elementwise_abs(tv);
        else dacc = __builtin_elementwise_fma(tv, tv, dacc);
      }
      const float dp_ = allsum_kq((dacc[0] + dacc[1]) + (dacc[2] + dacc[3]));
      if (kq == 0) dred[w * 16 + j] = dp_;
    }
  }
  __syncthreads();
  if (w == 0 && kq == 0) {                                       // the last tile's score
    const int64_t row0 = (tfirst + grp + (int64_t)(niter - 1) * tstride) * 16;
    if (row0 + j < a.n) (a.score + row0)[j] = (dred[j] + dred[16 + j]) + (dred[32 + j] + dred[48 + j]);
  }
}

template <typename G, bool L1>
int launch_fwd_wide_l(const McArgs& a, hipStream_t st, const char* name) {
  static_assert(G::TG >= 1, "LDS budget");
  const int64_t ntiles = (a.n + 15) / 16;
  int tg = ntiles >= 256 * 3 ? 3 : ntiles >= 256 * 2 ? 2 : 1;
  if (tg > G::TG) tg = G::TG;
  if (opt_fwd_wide() >= 2 && opt_fwd_wide() < tg) tg = opt_fwd_wide();      // (A/B: option fwd_wide = 2: two tile groups per workgroup)
  const size_t lds = G::TABLE_BYTES + (size_t)tg * G::GROUP_BYTES;
  (void)hipFuncSetAttribute((const void*)pref_fwd_wide_kernel<G, L1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(G::TABLE_BYTES + (size_t)G::TG * G::GROUP_BYTES));
  const int grid = grid_for((ntiles + tg - 1) / tg, 256);
  hipLaunchKernelGGL((pref_fwd_wide_kernel<G, L1>), dim3(grid), dim3(tg * 256), lds, st, a);
  return check_launch(name);
}

int launch_fwd_wide(const McArgs& a, int np, hipStream_t st, const char* name) {
#define KTUP_FW(NPV)                                                                                                  \
  {                                                                                                                   \
    if (a.E) return a.l1 ? launch_fwd_wide_l<FwGeom<NPV, true>, true>(a, st, name) : launch_fwd_wide_l<FwGeom<NPV, true>, false>(a, st, name);    \
    return a.l1 ? launch_fwd_wide_l<FwGeom<NPV, false>, true>(a, st, name) : launch_fwd_wide_l<FwGeom<NPV, false>, false>(a, st, name);           \
  }
  if (np <= 4) KTUP_FW(4)
  KTUP_FW(5)
#undef KTUP_FW
}

template <typename G, bool L1, bool BUF = false>
int launch_mc_l(const McArgs& a, hipStream_t st, const char* name) {
  static_assert(G::NW >= 2, "LDS budget");
  constexpr size_t lds = G::TABLE_BYTES + (size_t)G::NW * G::WAVE_BYTES;
  (void)hipFuncSetAttribute((const void*)pref_fwd_mc_kernel<G, L1, BUF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const int64_t ntiles = (a.n + 15) / 16;
  // small batches (a B = 512 training step is 64 tiles): fewer waves per workgroup, so that the tiles spread over many CUs
  // (one tile per SIMD) instead of queueing four deep on the matrix pipe of four CUs
  int nw = (int)((ntiles + 255) / 256);
  nw = nw < 4 ? (G::NW < 4 ? G::NW : 4) : (nw > G::NW ? G::NW : nw);
  const int grid = grid_for((ntiles + nw - 1) / nw, 256);
  hipLaunchKernelGGL((pref_fwd_mc_kernel<G, L1, BUF>), dim3(grid), dim3(nw * 64), lds, st, a);
  return check_launch(name);
}

template <typename G>
int launch_mc(const McArgs& a, hipStream_t st, const char* name) {
  if constexpr (G::NW < 2) {
    return 1;                                   // tables + one wave's tiles exceed the LDS: the caller's generic kernel runs
  } else {
    // option fwd_buf_gather: rows through buffer loads at 32-bit offsets (soft gate, d <= 128; the nontemporal hint is a compile-time
    // bit of a buffer load, and the tables it is for are the > 4 GB ones: nt_gather keeps the pointer kernel)
    if constexpr (!G::HARD && G::NCH <= 32) {
      if (opt_fwd_buf_gather() && !a.nt) return a.l1 ? launch_mc_l<G, true, true>(a, st, name) : launch_mc_l<G, false, true>(a, st, name);
    }
    return a.l1 ? launch_mc_l<G, true>(a, st, name) : launch_mc_l<G, false>(a, st, name);
  }
}

template <int NCH, int NP>
int launch_mc_e(const McArgs& a, hipStream_t st, const char* name) {
  if (a.gumbel != KTUP_GUMBEL_OFF) {
    if (a.E) return launch_mc<McGeom<NCH, NP, true, true>>(a, st, name);
    return launch_mc<McGeom<NCH, NP, false, true>>(a, st, name);
  }
  // option fwd_split: stage 2 on the bf16 matrix pipe, where that is fewer clocks (NP >= 4: six 16-clock MFMAs per tile and table
  // against NP 32-clock ones) and the three bf16 planes leave the workgroup as many waves as the fp32 tables do
  if constexpr (NCH <= 32 && NP >= 4 && McGeom<NCH, NP, true, false, SPLIT_SIX>::NW == McGeom<NCH, NP, true, false>::NW &&
                McGeom<NCH, NP, false, false, SPLIT_SIX>::NW == McGeom<NCH, NP, false, false>::NW) {
    if (opt_fwd_split()) {
      // option fwd_split_pack: at most five logits per lane (P <= 20) leave slots 5-7 of every k-quarter empty -- the six products packed
      // into four MFMAs (three at P <= 16) by ktup_split_plan.h; never more LDS than the six-product planes
      if constexpr (NP <= 5) {
        static_assert(McGeom<NCH, NP, true, false, SPLIT_PACK>::NW >= McGeom<NCH, NP, true, false, SPLIT_SIX>::NW &&
                      McGeom<NCH, NP, false, false, SPLIT_PACK>::NW >= McGeom<NCH, NP, false, false, SPLIT_SIX>::NW, "the packed planes fit where the six-product planes do");
        if (opt_fwd_split_pack()) {
          if (a.E) return launch_mc<McGeom<NCH, NP, true, false, SPLIT_PACK>>(a, st, name);
          return launch_mc<McGeom<NCH, NP, false, false, SPLIT_PACK>>(a, st, name);
        }
      }
      if (a.E) return launch_mc<McGeom<NCH, NP, true, false, SPLIT_SIX>>(a, st, name);
      return launch_mc<McGeom<NCH, NP, false, false, SPLIT_SIX>>(a, st, name);
    }
  }
  if (a.E) return launch_mc<McGeom<NCH, NP, true, false>>(a, st, name);
  return launch_mc<McGeom<NCH, NP, false, false>>(a, st, name);
}

template <int NCH>
int launch_mc_np(const McArgs& a, int np, hipStream_t st, const char* name) {
  if (np <= 2) return launch_mc_e<NCH, 2>(a, st, name);
  if (np <= 4) return launch_mc_e<NCH, 4>(a, st, name);
  if (np <= 5) return launch_mc_e<NCH, 5>(a, st, name);
  return launch_mc_e<NCH, 8>(a, st, name);
}

}  // namespace

// Returns KTUP_OK / an error, or 1 when (d, P) is not one of the instantiated geometries (the caller then runs the
// run-time-geometry kernel).
int pref_fwd_mc(const float* U, int64_t ldu, const float* I, int64_t ldi, const float* E, int64_t lde, const int32_t* item2ent,
                const float* Alog, const float* Ar, const float* Cn, int dp, int n_pref, int d, const int64_t* u_ids,
                const int64_t* i_ids, int64_t n, int l1, int gumbel_mode, const float* uniform, uint64_t seed, uint64_t offset,
                float* score, hipStream_t st, const char* name) {
  if (n_pref > 32 || (d != 64 && d != 100 && d != 128 && d != 256)) return 1;
  if ((ldu | ldi | lde) & 3) return 1;
  if ((ldu >> 2) > 0xffffffffll || (ldi >> 2) > 0xffffffffll || (lde >> 2) > 0xffffffffll) return 1;
  McArgs a;
  a.U = reinterpret_cast<const v4*>(U); a.I = reinterpret_cast<const v4*>(I); a.E = reinterpret_cast<const v4*>(E);
  a.ldu4 = (uint32_t)(ldu >> 2); a.ldi4 = (uint32_t)(ldi >> 2); a.lde4 = (uint32_t)(lde >> 2);
  a.item2ent = item2ent;
  a.Alog = Alog; a.Ar = Ar; a.Cn = Cn;
  a.dp = dp; a.P = n_pref; a.l1 = l1;
  a.gumbel = gumbel_mode; a.uniform = uniform; a.seed = seed; a.offset = offset;
  a.u_ids = u_ids; a.i_ids = i_ids; a.n = n; a.score = score; a.nt = opt_nt_gather();
  const int np = (n_pref + 3) / 4;
  if (d == 64) return launch_mc_np<16>(a, np, st, name);
  if (d == 100) return launch_mc_np<25>(a, np, st, name);
  if (d == 256) {
    // soft gate, P <= 20, more than a chip-load of tiles: the coordinate-split kernel (option fwd_wide); else 4 waves per CU, a tile each
    if (gumbel_mode == KTUP_GUMBEL_OFF && np <= 5 && n >= 16 * 256 && opt_fwd_wide()) return launch_fwd_wide(a, np, st, name);
    return launch_mc_np<64>(a, np, st, name);
  }
  return launch_mc_np<32>(a, np, st, name);
}

}  // namespace ktup
