// The packed split stage 2 of the soft-gate K5-K7 forward (ktup_score_pref_mc.hip), as data: which bf16 piece of which logit group sits
// in which of the 8 slots of a k-quarter, per MFMA, on both sides.  Host-compilable constexpr tables only -- the static_asserts at the
// end ARE the proof that the packing computes the six-product sum; the kernel's staging loop (A planes) and its B-operand assembly
// both read these tables and restate nothing.
//
// A table value a and a logit b are three bf16 pieces each (hi + mid + lo == x).  The six kept products per logit group s (a lane holds
// NS groups: preferences 4 s + kq) are hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi: 6 NS slot-products per k-quarter.  One
// v_mfma_f32_16x16x32_bf16 has 8 slots per k-quarter, so NS = 5 needs 30 slots = four MFMAs (six if every product class takes an
// MFMA of its own, slots 5-7 multiplying zeros) and NS <= 4 needs 24 = three.  An A plane is one LDS image of a table ([coordinate]
// [k-quarter][8 slots]); an MFMA names the plane it reads and its own B operand.  MFMAs are listed in issue order, smallest terms first.
#pragma once

namespace ktup {
namespace split_plan {

enum Piece : int { NONE = 0, HI = 1, MID = 2, LO = 3 };
struct Term {
  int piece, group;                     // group: the logit group s (preference 4 s + kq); NONE: the slot holds zero
};
struct Mfma {
  int plane;                            // which A plane this MFMA reads
  Term b[8];                            // its B operand, slot by slot
};
struct Plan {
  int ns, nplanes, nmfma;
  Term plane[3][8];                     // A planes, slot by slot
  Mfma mfma[4];                         // issue order
};

constexpr Term Z{NONE, 0};
constexpr Term H(int s) { return Term{HI, s}; }
constexpr Term M(int s) { return Term{MID, s}; }
constexpr Term L(int s) { return Term{LO, s}; }

// NS = 5 (16 < P <= 20), slots [0-4 | 5 | 6 | 7]:
//   d  Y = [al0..al4 | am4 | 0   | 0  ] x [bh0..bh4 | bm4 | 0   | 0  ]   lo.hi (all), mid.mid (4)
//   c  Z = [ah0..ah4 | am3 | am4 | am3] x [bl0..bl4 | bh3 | bh4 | bm3]   hi.lo (all), mid.hi (3, 4), mid.mid (3)
//   b  X = [ah0..ah4 | am0 | am1 | am2] x [bm0..bm4 | bm0 | bm1 | bm2]   hi.mid (all), mid.mid (0-2)
//   a  X                                x [bh0..bh4 | bh0 | bh1 | bh2]   hi.hi (all), mid.hi (0-2)
constexpr Plan PLAN5{5, 3, 4,
                     {/* X */ {H(0), H(1), H(2), H(3), H(4), M(0), M(1), M(2)},
                      /* Y */ {L(0), L(1), L(2), L(3), L(4), M(4), Z, Z},
                      /* Z */ {H(0), H(1), H(2), H(3), H(4), M(3), M(4), M(3)}},
                     {{1, {H(0), H(1), H(2), H(3), H(4), M(4), Z, Z}},
                      {2, {L(0), L(1), L(2), L(3), L(4), H(3), H(4), M(3)}},
                      {0, {M(0), M(1), M(2), M(3), M(4), M(0), M(1), M(2)}},
                      {0, {H(0), H(1), H(2), H(3), H(4), H(0), H(1), H(2)}}}};

// NS = 4 (12 < P <= 16), slots [0-3 | 4-7]:
//   c  Z = [ah | al] x [bl | bh]   hi.lo, lo.hi
//   b  X = [ah | am] x [bm | bm]   hi.mid, mid.mid
//   a  X             x [bh | bh]   hi.hi, mid.hi
constexpr Plan PLAN4{4, 2, 3,
                     {/* X */ {H(0), H(1), H(2), H(3), M(0), M(1), M(2), M(3)},
                      /* Z */ {H(0), H(1), H(2), H(3), L(0), L(1), L(2), L(3)},
                      {Z, Z, Z, Z, Z, Z, Z, Z}},
                     {{1, {L(0), L(1), L(2), L(3), H(0), H(1), H(2), H(3)}},
                      {0, {M(0), M(1), M(2), M(3), M(0), M(1), M(2), M(3)}},
                      {0, {H(0), H(1), H(2), H(3), H(0), H(1), H(2), H(3)}},
                      {0, {Z, Z, Z, Z, Z, Z, Z, Z}}}};

// NS = 3 (8 < P <= 12): the same with slots 3 and 7 empty
constexpr Plan PLAN3{3, 2, 3,
                     {/* X */ {H(0), H(1), H(2), Z, M(0), M(1), M(2), Z},
                      /* Z */ {H(0), H(1), H(2), Z, L(0), L(1), L(2), Z},
                      {Z, Z, Z, Z, Z, Z, Z, Z}},
                     {{1, {L(0), L(1), L(2), Z, H(0), H(1), H(2), Z}},
                      {0, {M(0), M(1), M(2), Z, M(0), M(1), M(2), Z}},
                      {0, {H(0), H(1), H(2), Z, H(0), H(1), H(2), Z}},
                      {0, {Z, Z, Z, Z, Z, Z, Z, Z}}}};

constexpr const Plan& plan_for(int ns) { return ns >= 5 ? PLAN5 : ns == 4 ? PLAN4 : PLAN3; }

// the A side of (MFMA m, slot k)
constexpr Term a_term(const Plan& p, int m, int k) { return p.plane[p.mfma[m].plane][k]; }

// product class of a slot: 0 hi.hi, 1 hi.mid, 2 mid.hi, 3 mid.mid, 4 hi.lo, 5 lo.hi; -1 for an empty slot, -2 for anything else
constexpr int product_class(Term a, Term b) {
  if (a.piece == NONE && b.piece == NONE) return -1;
  if (a.piece == HI && b.piece == HI) return 0;
  if (a.piece == HI && b.piece == MID) return 1;
  if (a.piece == MID && b.piece == HI) return 2;
  if (a.piece == MID && b.piece == MID) return 3;
  if (a.piece == HI && b.piece == LO) return 4;
  if (a.piece == LO && b.piece == HI) return 5;
  return -2;
}

// every (product class, group) of the six classes exactly once
constexpr bool each_product_once(const Plan& p) {
  for (int cls = 0; cls < 6; ++cls)
    for (int s = 0; s < p.ns; ++s) {
      int n = 0;
      for (int m = 0; m < p.nmfma; ++m)
        for (int k = 0; k < 8; ++k)
          if (product_class(a_term(p, m, k), p.mfma[m].b[k]) == cls && a_term(p, m, k).group == s) ++n;
      if (n != 1) return false;
    }
  return true;
}
// no slot pairs pieces of different groups, no group past NS, no product outside the six classes
constexpr bool groups_match(const Plan& p) {
  for (int m = 0; m < p.nmfma; ++m)
    for (int k = 0; k < 8; ++k) {
      const Term a = a_term(p, m, k), b = p.mfma[m].b[k];
      const int cls = product_class(a, b);
      if (cls == -2) return false;
      if (cls >= 0 && (a.group != b.group || a.group < 0 || a.group >= p.ns)) return false;
    }
  return true;
}
// a slot is empty on both sides or on neither; planes and MFMAs past the counts hold nothing
constexpr bool unused_are_zero(const Plan& p) {
  for (int m = 0; m < 4; ++m)
    for (int k = 0; k < 8; ++k) {
      const Term b = p.mfma[m].b[k];
      if (m >= p.nmfma) {
        if (b.piece != NONE) return false;
        continue;
      }
      if ((a_term(p, m, k).piece == NONE) != (b.piece == NONE)) return false;
    }
  for (int pl = p.nplanes; pl < 3; ++pl)
    for (int k = 0; k < 8; ++k)
      if (p.plane[pl][k].piece != NONE) return false;
  return true;
}
constexpr bool planes_ok(const Plan& p) {
  if (p.nplanes < 1 || p.nplanes > 3 || p.nmfma < 1 || p.nmfma > 4) return false;
  for (int m = 0; m < p.nmfma; ++m)
    if (p.mfma[m].plane < 0 || p.mfma[m].plane >= p.nplanes) return false;
  return true;
}
// what the kernel's B-operand assembly leans on: the last MFMA's B operand is made of hi pieces alone, with group s in slot s (s < NS),
// and the one before it of hi and mid pieces, with the mid piece of group s in slot s -- the residues x - hi and x - hi - mid are
// taken from those two operands, so neither needs a residue that is not there yet
constexpr bool levels_in_place(const Plan& p) {
  if (p.nmfma < 2) return false;
  for (int s = 0; s < p.ns; ++s) {
    const Term h = p.mfma[p.nmfma - 1].b[s], m = p.mfma[p.nmfma - 2].b[s];
    if (h.piece != HI || h.group != s || m.piece != MID || m.group != s) return false;
  }
  for (int k = 0; k < 8; ++k) {
    if (p.mfma[p.nmfma - 1].b[k].piece == MID || p.mfma[p.nmfma - 1].b[k].piece == LO) return false;
    if (p.mfma[p.nmfma - 2].b[k].piece == LO) return false;
  }
  return true;
}
constexpr bool valid(const Plan& p) {
  return planes_ok(p) && groups_match(p) && unused_are_zero(p) && each_product_once(p) && levels_in_place(p);
}

static_assert(PLAN3.ns == 3 && PLAN4.ns == 4 && PLAN5.ns == 5, "one plan per number of logits a lane holds");
static_assert(planes_ok(PLAN3) && planes_ok(PLAN4) && planes_ok(PLAN5), "at most three A planes per table, four MFMAs");
static_assert(groups_match(PLAN3) && groups_match(PLAN4) && groups_match(PLAN5), "a slot pairs pieces of ONE logit group, in one of the six classes");
static_assert(unused_are_zero(PLAN3) && unused_are_zero(PLAN4) && unused_are_zero(PLAN5), "an unused slot is zero on both sides");
static_assert(each_product_once(PLAN3) && each_product_once(PLAN4) && each_product_once(PLAN5),
              "every (product class, group) of hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi occurs exactly once");
static_assert(levels_in_place(PLAN3) && levels_in_place(PLAN4) && levels_in_place(PLAN5), "hi / mid pieces of group s in slot s of the last two MFMAs");
static_assert(PLAN5.nmfma == 4 && PLAN4.nmfma == 3 && PLAN3.nmfma == 3, "30 slot-products in four MFMAs, 24 / 18 in three");

}  // namespace split_plan
}  // namespace ktup
