// gmr_ik_tree.h -- the box-QP of one IK solve, factorised along the kinematic tree by FOUR wavefronts.
//
// H = damping I + sum_k J_k^T W^2 J_k couples two dofs only if one is an ancestor of the other
// (a task's Jacobian lives on its root->frame path).  Ordered limbs-first, H is block-arrowhead:
//
//        [ D_1            B_1^T ]      D_l : dofs of limb l (a chain: dense, <= 8)
//    H = [      ...        ...  ]      T   : trunk dofs (floating base, waist, short appendages: <= 10)
//        [            D_4 B_4^T ]      B_l : trunk x limb coupling
//        [ B_1  ...  B_4   T    ]
//
// Each wavefront eliminates ONE limb (Cholesky of D_l, Y_l = B_l L_l^-T, its Schur contribution
// -Y_l Y_l^T and the forward-substituted right-hand side) with its rows in registers exactly like the
// dense solver, but on an 18-column local matrix: 108 instead of 630 (pivot, column) updates and 8
// instead of 36 pivots on the critical path, the four limbs side by side.  Every wavefront then sums,
// factors and solves the trunk Schur complement redundantly (no exchange of x_T), and the limbs
// back-substitute in parallel.  The rows are FULL symmetric rows: the right-looking elimination updates every
// column of every lane and leaves a finished row alone, so at its pivot lane p holds row p of the unscaled upper
// factor, and one multiply by its own 1 / sqrt(d_p) gives column p of the lower factor -- the operand of the back
// substitutions -- bit for bit what the lanes below hold (H is bitwise symmetric; a fused update multiplies the same
// two numbers in either lane).  No factor is transposed through LDS.
// Bounds are handled by the same block principal pivoting as the dense solver (gmr_ik.hip) on wave-uniform bound masks kept identically in all wavefronts: two to three workgroup
// barriers per pivoting round (Schur parts; the limbs' shares of a fixed trunk row's multiplier; violation sets).
//
// Used by the latency shape (NW = 4) when the robot decomposes into <= 4 limbs of <= 8 dofs and a
// trunk of <= 10 (all 8 shipped robots do); other robots always run the 1-wavefront kernel (dense solver).
#pragma once
#include <type_traits>

namespace gmr {

constexpr int TR_MAX_NL = 8;                     // capacity: limb rows per wavefront (LDS tables)
constexpr int TR_MAX_NT = 10;                    // capacity: trunk rows

// The exchange buffers of a round (Spart, rpart, gpart) start on 16-byte boundaries (gmr_ik_layout.h) and a row of Spart
// is 80 B: two neighbouring columns are one 16-byte piece.  GMR_NO_ALIGNED_SCHUR restores the 8-byte accesses (A/B builds).
struct __attribute__((aligned(16))) TrPair { double x, y; };
#ifdef GMR_NO_ALIGNED_SCHUR
constexpr bool TR_PAIRS = false;
#else
constexpr bool TR_PAIRS = true;
#endif
// The masks of a round as lane masks: an entry of the local matrix is kept where the lane's row is free (one lane mask per
// round) and the column is free (a wave-uniform bit of the round's ballot), and the 1.0 on the diagonal of a fixed or padding
// row is not written into the row: the pivot's diagonal broadcast takes it from the column's bit (solve_qp_tree, TR_DIAG).
// GMR_NO_LANE_MASKS restores the per-entry identity (A/B builds).
#ifdef GMR_NO_LANE_MASKS
constexpr bool TR_LMASK = false;
#else
constexpr bool TR_LMASK = true;
#endif

// Bound sets of the QP, identical in every wavefront (wave-uniform registers, carried from solve to
// solve for the warm start): bit d of `lower` / `upper` = dof d sits on its lower / upper bound.
struct TreeState { unsigned long long lower, upper; };

// All four wavefronts call this together.  Returns GMR_STATUS_* (the same value in every wavefront);
// the solution is left in sm[L.o.x].  Two workgroup barriers per pivoting round (three when a TRUNK variable
// sits on a bound): the trunk system is summed, factorised and solved redundantly by every wavefront, so
// the only exchanges are the limbs' Schur contributions, the violation sets and -- for the multiplier of a fixed
// trunk variable -- each limb's share of that row of H x.  Row i of H is structurally zero outside its own limb and
// the trunk: exactly the columns of the local matrix of the wavefront that owns the row, which holds their x in
// lanes 0 .. TR_NV-1 after the back substitution.  The multiplier of a fixed LIMB variable is therefore formed from
// registers alone (TR_NV row broadcasts and FMAs); nobody reads sm[L.o.x] inside a round.
// The same structure forms the RIGHT-HAND SIDE of a round with fixed variables, -c_i - sum over fixed j of H_ij x_j:
// column m of the local matrix is the dof of lane m, so the bound value of column m is a broadcast of lane m's `xfix`
// (an exact zero for a free or padding lane), and the sum runs over the TR_NV columns in a fixed order that does not
// depend on the bound set: the limb columns' products in two FMA chains by column parity (even + odd), the trunk
// columns' likewise.  A free limb row subtracts both sums from -c_i.  A free trunk row keeps the trunk columns' sum in
// its own right-hand side and starts its forward-substituted share `b` from minus the sum over THIS wavefront's limb
// columns; the share reaches the trunk system through `rpart`, which every wavefront adds as (w0 + w1) + (w2 + w3), and
// elimination leaves it alone (a fixed limb column's pivot has l = 0 in every other row).  No loop over the set bits of
// the bound masks, no read of lo / hi.
// The unmasked row of H over the local matrix' columns (clamped address for a padding column: finite, multiplied by
// zeros or masked) is read ONCE per solve into registers -- H does not change between the rounds of a solve -- and
// serves the row build, these products, the trunk rows and the multipliers.
// TR_NL / TR_NT: rows actually eliminated (limbs <= TR_NL dofs, trunk <= TR_NT): the pivots are unrolled, so a
// robot with 7-dof limbs and a 9-dof trunk (every shipped one) runs the <7, 9> instance: 16 instead of 18 pivots.
//
// ROWS = true: the same algorithm inside ONE wavefront (the 1-wavefront launch shape).  The four limbs occupy
// the four 16-lane DPP rows of the wave (TR_NL + TR_NT <= 16: 7 limb rows + 9 trunk rows), "wavefront" becomes
// "row", v_readlane broadcasts become DPP row broadcasts (one instruction pair serves all four limbs; the
// result stays in a VGPR), workgroup barriers become LDS fences.  Replaces the dense 36-pivot factorisation
// of the throughput shape for robots that fit.
// What a wavefront reads from the decomposition tables for every solve: the dof of its row and the (wave-uniform) dofs
// of its local matrix' columns.  They never change during a launch: read once (tree_rows), kept in registers.
template <int TR_NV>
struct TreeRows { int dof; int cdof[TR_NV]; };

template <int TR_NL, int TR_NT, bool ROWS, class LT>
__device__ __forceinline__ TreeRows<TR_NL + TR_NT> tree_rows(const LT& L, const short* si, int wave_in, int lane_in) {
  const int wave = ROWS ? (lane_in >> 4) : wave_in, lane = ROWS ? (lane_in & 15) : lane_in;
  const short* limb = si + L.o.i_tree_limb + wave * TR_MAX_NL;
  const short* trunk = si + L.o.i_tree_trunk;
  TreeRows<TR_NL + TR_NT> R;
  R.dof = lane < TR_NL ? limb[lane] : (lane < TR_NL + TR_NT ? trunk[lane - TR_NL] : -1);
#pragma unroll
  for (int m = 0; m < TR_NL; m++) R.cdof[m] = limb[m];
#pragma unroll
  for (int u = 0; u < TR_NT; u++) R.cdof[TR_NL + u] = trunk[u];
  return R;
}

// f(integral_constant<int, I>) for I = I0 .. I1 - 1: the pivots as compile-time constants (the folded row broadcasts
// of gmr_device_math.h take their lane as an immediate)
template <int I0, int I1, class F>
__device__ __forceinline__ void tr_static_for(F&& f) {
  if constexpr (I0 < I1) {
    f(std::integral_constant<int, I0>{});
    tr_static_for<I0 + 1, I1>(f);
  }
}

template <int TR_NL, int TR_NT, bool ROWS, bool DPPB, class LT>
__device__ __forceinline__ int solve_qp_tree(const LT& L, double* sm, uint32_t* sw, const short* si, int wave_in,
                                             int lane_in, TreeState& bs, Prof& pr, const TreeRows<TR_NL + TR_NT>& rows) {
  constexpr int TR_NV = TR_NL + TR_NT;             // local matrix order
  static_assert(!ROWS || TR_NV <= 16, "a limb's local matrix must fit one 16-lane row");
  const int wave = ROWS ? (lane_in >> 4) : wave_in;        // which limb this wavefront / row eliminates
  const int lane0 = ROWS ? (lane_in & 15) : lane_in;       // row of the local matrix
  // Every phase below starts from a FRESH copy of the row index (fresh_lane, gmr_device_math.h): its lane predicates
  // (row == pivot, row > pivot, ...) are recomputed where they are used and die with the phase, instead of being
  // computed once per kernel and parked in (spilled) SGPR pairs.
#define TR_ROW()                                                                                   \
  const int lane = fresh_lane(lane0);                                                              \
  const bool is_limb = lane < TR_NL, is_trunk = lane >= TR_NL && lane < TR_NV;                     \
  const int a = lane, t = lane - TR_NL;                                                            \
  (void)is_limb; (void)is_trunk; (void)a; (void)t;
  const int lane = lane0;
  static_assert(!DPPB || TR_NV <= 16, "DPP row broadcasts need the local matrix in one 16-lane row");
#define TR_BCAST(v, k) ((ROWS || DPPB) ? row_bcast_d((v), (k)) : readlane_d((v), (k)))
  // DPP broadcasts that feed a multiply-add are folded into it (row_bcast_fma and its multi-update forms: the same
  // fused operation on the same three numbers); the v_readlane path of the <8, 10> instance keeps fma(.., TR_BCAST(..), ..)
  constexpr bool FOLD = ROWS || DPPB;
  // ... and a pivot, a back substitution is ONE statement that covers its own DPP wait states (row_bcast_fnma_pivot,
  // row_backsub_fill, row_dot_backsub: the same operations on the same operands in the same order per row; the <7, 9> shape)
#ifdef GMR_NO_FILLED_WAITS
  constexpr bool FILLED = false;
#else
  constexpr bool FILLED = FOLD && TR_NL == 7 && TR_NT == 9;
#endif
  // the diagonal a pivot sees: column k of a fixed or padding row k is the identity (colmask: wave-uniform, ROWS: per row)
#define TR_DIAG(d, k) ((TR_LMASK && ((colmask >> (k)) & 1u)) ? 1.0 : (d))
#define TR_SYNC() do { if (ROWS) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); else __syncthreads(); } while (0)
  const int n = L.nv, ldh = L.o.ldh;
  const double* H = sm + L.o.H;
  double* xs = sm + L.o.x;
  const double* los = sm + L.o.lo;
  const double* his = sm + L.o.hi;
  static_assert(!TR_PAIRS || (LT::o.tr_spart % 2 == 0 && TR_MAX_NT % 2 == 0), "rows of the Schur parts start on 16-byte boundaries");
  double* Spart = sm + L.o.tr_spart;                           // [4][TR_NT][TR_NT]
  double* rpart = sm + L.o.tr_rpart;                           // [4][TR_NT]
  double* gpart = sm + L.o.tr_gpart;                           // [4][TR_NT] (4-wavefront form only)
  // violation sets of a round, double-buffered: {to_lower, to_upper, release, flags} x 2
  unsigned long long* vset = reinterpret_cast<unsigned long long*>(sw + L.o.w_tr_mask);

  const bool is_limb = lane < TR_NL, is_trunk = lane >= TR_NL && lane < TR_NV;
  const int a = lane, t = lane - TR_NL;
  const int dof = rows.dof;                                  // dof of limb row a / trunk row t, or -1
  const bool row = dof >= 0;                                 // this lane holds a real row
  const bool own = row && (is_limb || wave == 0);            // ... and reports the variable's violations
  const double lo = row ? los[dof] : 0.0, hi = row ? his[dof] : 0.0;
  const double ci = row ? (sm + L.o.c)[dof] : 0.0;
  const double* Hrow = H + (row ? dof : 0) * ldh;
  double dual_tol = -1.0;                                      // 1e-13 (1 + max |c|): computed when a multiplier is first checked
  const double ptol_lo = 1e-12 * (1.0 + fabs(lo)), ptol_hi = 1e-12 * (1.0 + fabs(hi));
  // column dofs of the local matrix (wave-uniform): limb columns then trunk columns
  const int* cdof = rows.cdof;

  // row `dof` of H over the local matrix' columns, unmasked (a padding column reads column 0: finite, never used unmasked)
  double h[TR_NV];
#pragma unroll
  for (int m = 0; m < TR_NV; m++) h[m] = Hrow[cdof[m] >= 0 ? cdof[m] : 0];

  int pcount = 3, ninf_best = 65;
  for (int it = 0; it < 100; it++) {
    PROF_COUNT(pr, PH_NFACT);                                 // pivoting rounds (one factorisation each)
    PROF_BEGIN(pr);
    const unsigned long long fixedm = bs.lower | bs.upper;
    const bool self_fixed = !row || ((fixedm >> dof) & 1ull);
    const double xfix = !row ? 0.0 : (((bs.lower >> dof) & 1ull) ? lo : (((bs.upper >> dof) & 1ull) ? hi : 0.0));
    // Column m of the local matrix is the dof of lane m: "column m is fixed or padding" is lane m's self_fixed.  One
    // ballot per round holds all TR_NV of them at constant bit positions (ROWS: in the 16-bit slice of the lane's row).
    const unsigned long long fixed_lanes = __ballot(self_fixed);
    const unsigned colmask = (ROWS ? (unsigned)(fixed_lanes >> (16 * wave)) : (unsigned)fixed_lanes) & ((1u << TR_NV) - 1u);
    // ---- (1) local rows and right-hand side -----------------------------------------------------
    double r[TR_NV];
#pragma unroll
    for (int m = 0; m < TR_NV; m++) r[m] = 0.0;
    double rhs0, b;
    {
    TR_ROW()
#pragma unroll
    for (int m = 0; m < TR_NL; m++) {
      const bool cfixed = (colmask >> m) & 1u;                // wave-uniform (ROWS: uniform in the 16-lane row)
      // every free row keeps all its free limb columns: D_l as full symmetric rows (limb rows), B_l (trunk rows)
      const bool keep = row && !self_fixed && !cfixed;
      double v = keep ? h[m] : 0.0;
      // fixed / padding limb row: identity.  TR_LMASK: its diagonal stays zero here; it is read only by the pivot's diagonal
      // broadcast (TR_DIAG) -- l is zero for rows <= pivot, ltl takes the columns beyond the diagonal only
      if (!TR_LMASK && is_limb && m == a && (self_fixed || cfixed)) v = 1.0;
      r[m] = v;
    }
    // limb row a also keeps its trunk columns, B_l^T: column a of Y_l grows there.  (A trunk row's trunk columns start
    // from zero and collect its Schur part.)
#pragma unroll
    for (int u = 0; u < TR_NT; u++) {
      const bool cfixed = (colmask >> (TR_NL + u)) & 1u;      // wave-uniform
      r[TR_NL + u] = (is_limb && row && !self_fixed && !cfixed) ? h[TR_NL + u] : 0.0;
    }
    // -c_i - sum over fixed j of H_ij x_j: lane m's xfix is the bound value of column m (0.0 when free or padding), so
    // every product of a column that is not fixed is an exact zero.  Fixed order, two chains per part (header comment).
    rhs0 = row ? (self_fixed ? xfix : -ci) : 0.0;
    double bshare = 0.0;                                      // free trunk row: its limb columns' part, sent through rpart
    if (fixedm != 0ull) {                                     // (wave-uniform; most solves never fix a variable)
      double sl0 = 0.0, sl1 = 0.0, st0 = 0.0, st1 = 0.0;
      if constexpr (FOLD) {
        sl0 = row_bcast_fma_dot<0, 2, (TR_NL + 1) / 2, false>(sl0, xfix, h);
        sl1 = row_bcast_fma_dot<1, 2, TR_NL / 2, false>(sl1, xfix, h + 1);
        st0 = row_bcast_fma_dot<TR_NL, 2, (TR_NT + 1) / 2, false>(st0, xfix, h + TR_NL);
        st1 = row_bcast_fma_dot<TR_NL + 1, 2, TR_NT / 2, false>(st1, xfix, h + TR_NL + 1);
      } else {
#pragma unroll
        for (int m = 0; m < TR_NL; m++) {
          const double xf = TR_BCAST(xfix, m);
          if (m & 1) sl1 = fma(h[m], xf, sl1); else sl0 = fma(h[m], xf, sl0);
        }
#pragma unroll
        for (int u = 0; u < TR_NT; u++) {
          const double xf = TR_BCAST(xfix, TR_NL + u);
          if (u & 1) st1 = fma(h[TR_NL + u], xf, st1); else st0 = fma(h[TR_NL + u], xf, st0);
        }
      }
      const double sl = sl0 + sl1, st = st0 + st1;
      if (row && !self_fixed) {
        rhs0 = is_limb ? (rhs0 - st) - sl : rhs0 - st;
        bshare = -sl;
      }
    }
    b = is_limb ? rhs0 : (is_trunk ? bshare : 0.0);
    }
    PROF_END(pr, PH_KBUILD);
    PROF_BEGIN(pr);
    // ---- (2) eliminate the limb pivots (right-looking, forward substitution merged) --------------
    // The next pivot's column is updated first and its reciprocal square root started at once, so
    // that the Newton steps overlap the remaining (independent) column updates of this pivot.
    double mydinv = 1.0;
    bool bad = false;
    double dp = TR_DIAG(TR_BCAST(r[0], 0), 0);
    double dinv = fast_rsqrt(dp);
    tr_static_for<0, TR_NL>([&](auto P) __attribute__((always_inline)) {
      constexpr int p = decltype(P)::value;
      const int lane = fresh_lane(lane0);                    // (lane > p), (lane == p): computed here, dead after this pivot
      bad = bad || !(dp > 0.0);
      const double rs = r[p] * dinv;                         // (row p holds the pivot itself: d_p / sqrt(d_p))
      double l = lane > p ? rs : 0.0;                        // column p of L_l (rows > p) and of Y_l
      if (lane == p) mydinv = dinv;                          // (rows <= p keep r[p]: l = 0 leaves a finished row alone)
      double dinv_next = 1.0;
      if constexpr (p + 1 < TR_NL) {
        if constexpr (FILLED) {                              // all columns of the pivot, the new diagonal broadcast behind them
          dp = row_bcast_fnma_pivot<p + 1, TR_NV - p - 1>(r + p + 1, l);
        } else if constexpr (FOLD) {
          dp = row_bcast_fnma_bcast<p + 1>(r[p + 1], l);
        } else {
          r[p + 1] = fma(-l, TR_BCAST(l, p + 1), r[p + 1]);
          dp = TR_BCAST(r[p + 1], p + 1);
        }
        dp = TR_DIAG(dp, p + 1);
        dinv_next = fast_rsqrt(dp);
      }
      const double yp = TR_BCAST(b, p) * dinv;               // row p keeps its unscaled b (l = 0 there): scaled after the loop
      b = fma(-l, yp, b);
      constexpr int k0 = p + 1 < TR_NL ? p + 2 : p + 1;
      if constexpr (FILLED && p + 1 < TR_NL) {
      } else if constexpr (FOLD) {
        row_bcast_fnma_cols<k0, TR_NV - k0>(r + k0, l);
      } else {
#pragma unroll
        for (int k = k0; k < TR_NV; k++) r[k] = fma(-l, TR_BCAST(l, k), r[k]);
      }
      dinv = dinv_next;
    });
    if (fresh_lane(lane0) < TR_NL) b *= mydinv;              // y_p = b_p / sqrt(d_p): the value every later row was given
    // Operands of the limb back substitution (5): column a of L_l without its diagonal and of Y_l.  The local matrix is
    // symmetric, so when pivot a came, limb lane a held row a of the unscaled upper factor in r[k], k > a -- entry (a, k)
    // started equal to entry (k, a) of lane k and received the same fused updates at pivots 0 .. a-1 -- and nothing
    // touched it since.  Scaled by the lane's own 1 / sqrt(d_a) it is column a of the lower factor, bit for bit what
    // lane k holds in its column a: no transpose through LDS.
    // FILLED: the sixteen products are the wait states of the trunk back substitution (4), the selects follow it.
    double ltl[TR_NL], yl[TR_NT];
    if constexpr (!FILLED) {
      TR_ROW()
#pragma unroll
      for (int m = 0; m < TR_NL; m++) ltl[m] = (is_limb && m > a) ? r[m] * mydinv : 0.0;
#pragma unroll
      for (int u = 0; u < TR_NT; u++) yl[u] = r[TR_NL + u] * mydinv;   // (used by limb lanes only)
    }
    PROF_END(pr, PH_CHOL);
    PROF_BEGIN(pr);
    // ---- (3) publish the Schur contribution --------------------------------------------------------
    unsigned long long* vcur = vset + 4 * (it & 1);
    {
    TR_ROW()
    if (is_trunk) {
      double* srow = Spart + (wave * TR_MAX_NT + t) * TR_MAX_NT;
#pragma unroll
      for (int u = 0; u < TR_NT; u++) {
        if (TR_PAIRS && u + 1 < TR_NT && !(u & 1)) *reinterpret_cast<TrPair*>(srow + u) = TrPair{r[TR_NL + u], r[TR_NL + u + 1]};
        else if (!(TR_PAIRS && (u & 1))) srow[u] = r[TR_NL + u];
      }
      rpart[wave * TR_MAX_NT + t] = b;
    }
    if (lane == 0 && bad) atomicOr(&vcur[3], 1ull);
    TR_SYNC();                                                                               // B1
    // the other slot was last read before this barrier: clear it for the next round
    if (wave == 0 && lane < 4) vset[4 * ((it + 1) & 1) + lane] = 0ull;
    }
    PROF_END(pr, PH_SUBST);
    PROF_BEGIN(pr);
    // ---- (4) every wavefront: trunk Schur complement, factor, solve (redundant, no exchange) -------
    double bt = 0.0;
    bool tbad = false;
    {
      double s[TR_NT];
#pragma unroll
      for (int u = 0; u < TR_NT; u++) s[u] = 0.0;
      {
        TR_ROW()
        // all loads first (clamped addresses, no branches), then the masks
        const int tt = is_trunk ? t : 0;
        double hv[TR_NT], sp[TR_NT];
#pragma unroll
        for (int u = 0; u < TR_NT; u++) hv[u] = h[TR_NL + u];
        if constexpr (TR_PAIRS) {
          // the row of each part as 16-byte pieces from one address (TR_NT odd: the last piece's second half is the
          // row's unused column TR_NT < TR_MAX_NT, read and dropped)
          constexpr int PART = TR_MAX_NT * TR_MAX_NT / 2;
          const TrPair* q0 = reinterpret_cast<const TrPair*>(Spart + tt * TR_MAX_NT);
#pragma unroll
          for (int j = 0; j < (TR_NT + 1) / 2; j++) {
            const TrPair p0 = q0[j], p1 = q0[PART + j], p2 = q0[2 * PART + j], p3 = q0[3 * PART + j];
            sp[2 * j] = (p0.x + p1.x) + (p2.x + p3.x);
            if (2 * j + 1 < TR_NT) sp[2 * j + 1] = (p0.y + p1.y) + (p2.y + p3.y);
          }
        } else {
#pragma unroll
          for (int u = 0; u < TR_NT; u++) {
            const double* q0 = Spart + tt * TR_MAX_NT + u;
            sp[u] = (q0[0] + q0[TR_MAX_NT * TR_MAX_NT]) + (q0[2 * TR_MAX_NT * TR_MAX_NT] + q0[3 * TR_MAX_NT * TR_MAX_NT]);
          }
        }
        const double rp = (rpart[tt] + rpart[TR_MAX_NT + tt]) + (rpart[2 * TR_MAX_NT + tt] + rpart[3 * TR_MAX_NT + tt]);
        const bool live = is_trunk && row && !self_fixed;
#pragma unroll
        for (int u = 0; u < TR_NT; u++) {
          const bool cfixed = (colmask >> (TR_NL + u)) & 1u;               // wave-uniform
          double v = (live && !cfixed) ? hv[u] + sp[u] : 0.0;       // full symmetric rows, as in (1)
          if (!TR_LMASK && is_trunk && u == t && !(live && !cfixed)) v = 1.0;   // (TR_LMASK: TR_DIAG, as in (1))
          s[u] = v;
        }
        bt = is_trunk ? (live ? rhs0 + rp : rhs0) : 0.0;
      }
      double tdinv = 1.0;
      double dq = TR_DIAG(TR_BCAST(s[0], TR_NL), TR_NL);
      double dinv = fast_rsqrt(dq);
      tr_static_for<0, TR_NT>([&](auto Q) __attribute__((always_inline)) {
        constexpr int q = decltype(Q)::value;
        const int t = fresh_lane(lane0) - TR_NL;             // (t > q), (t == q): computed here, dead after this pivot
        tbad = tbad || !(dq > 0.0);
        const double ss = s[q] * dinv;
        double l = t > q ? ss : 0.0;
        if (t == q) tdinv = dinv;                            // (rows <= q keep s[q], as in (2))
        double dinv_next = 1.0;
        if constexpr (q + 1 < TR_NT) {
          if constexpr (FILLED) {
            dq = row_bcast_fnma_pivot<TR_NL + q + 1, TR_NT - q - 1>(s + q + 1, l);
          } else if constexpr (FOLD) {
            dq = row_bcast_fnma_bcast<TR_NL + q + 1>(s[q + 1], l);
          } else {
            s[q + 1] = fma(-l, TR_BCAST(l, TR_NL + q + 1), s[q + 1]);
            dq = TR_BCAST(s[q + 1], TR_NL + q + 1);
          }
          dq = TR_DIAG(dq, TR_NL + q + 1);
          dinv_next = fast_rsqrt(dq);
        }
        const double yq = TR_BCAST(bt, TR_NL + q) * dinv;
        bt = fma(-l, yq, bt);
        if constexpr (FILLED) {
        } else if constexpr (FOLD && q + 2 < TR_NT) {
          row_bcast_fnma_cols<TR_NL + q + 2, TR_NT - q - 2>(s + q + 2, l);
        } else {
#pragma unroll
          for (int k = q + 2; k < TR_NT; k++) s[k] = fma(-l, TR_BCAST(l, TR_NL + k), s[k]);
        }
        dinv = dinv_next;
      });
      // back substitution: row t of L^T without its diagonal is trunk lane t's own unscaled upper row times its
      // 1 / sqrt(d_t), as in (2) (the rows below are zero, rows outside the trunk get zeros): row q is final when its
      // step comes, so no step needs a select
      double lt[TR_NT];
      {
        TR_ROW()
#pragma unroll
        for (int q = 0; q < TR_NT; q++) lt[q] = (is_trunk && q > t) ? s[q] * tdinv : 0.0;
      }
      bt *= tdinv;                                           // y (rows kept their unscaled right-hand side)
      if constexpr (FILLED) {
        // one statement; its wait states are r[k] *= mydinv, the operands of (5): Y_l (trunk columns) and, behind their
        // selects, L_l^T (limb columns)
        if constexpr (TR_NL == 7 && TR_NT == 9) {            // (the statement is written out for this shape)
          double f[TR_NV];
#pragma unroll
          for (int j = 0; j < TR_NV; j++) f[j] = r[(TR_NL + j) % TR_NV];
          bt = row_backsub_fill<TR_NL>(bt, tdinv, lt, f, mydinv);
          TR_ROW()
#pragma unroll
          for (int u = 0; u < TR_NT; u++) yl[u] = f[u];      // (used by limb lanes only)
#pragma unroll
          for (int m = 0; m < TR_NL; m++) ltl[m] = (is_limb && m > a) ? f[TR_NT + m] : 0.0;
        }
      } else if constexpr (FOLD) {
        tr_static_for<0, TR_NT>([&](auto I) __attribute__((always_inline)) {
          constexpr int q = TR_NT - 1 - decltype(I)::value;
          bt = row_bcast_fma<TR_NL + q, true>(bt, bt * tdinv, lt[q]);
        });
      } else {
#pragma unroll
        for (int q = TR_NT - 1; q >= 0; q--) {
          const double xq = TR_BCAST(bt * tdinv, TR_NL + q);
          bt = fma(-lt[q], xq, bt);
        }
      }
      bt *= tdinv;                                           // x
    }
    PROF_END(pr, PH_RATIO);
    PROF_BEGIN(pr);
    // ---- (5) limbs: y_l - Y_l^T x_T, then back substitution with L_l^T ----------------------------
    double x = bt;                                                                     // trunk lanes
    {
      double bb = b;                                                                   // y_l (limb lanes)
      if constexpr (FILLED) {
        if constexpr (TR_NL == 7 && TR_NT == 9) bb = row_dot_backsub<TR_NL, 0>(bb, bt, yl, mydinv, ltl);
      } else if constexpr (FOLD) {
        // unconditional: a trunk lane's bb is dead (its x is bt, and the back substitution reads limb lanes only)
        bb = row_bcast_fma_dot<TR_NL, 1, TR_NT, true>(bb, bt, yl);                     // Y_l[u][a]
        tr_static_for<0, TR_NL>([&](auto I) __attribute__((always_inline)) {
          constexpr int p = TR_NL - 1 - decltype(I)::value;
          bb = row_bcast_fma<p, true>(bb, bb * mydinv, ltl[p]);   // (rows >= p have ltl[p] = 0: row p is final at its step)
        });
      } else {
        {
          TR_ROW()
#pragma unroll
          for (int u = 0; u < TR_NT; u++) {
            const double xt = TR_BCAST(bt, TR_NL + u);
            if (is_limb) bb = fma(-yl[u], xt, bb);                                     // Y_l[u][a]
          }
        }
#pragma unroll
        for (int p = TR_NL - 1; p >= 0; p--) {
          const double xp = TR_BCAST(bb * mydinv, p);
          bb = fma(-ltl[p], xp, bb);                         // (rows >= p have ltl[p] = 0: row p is final at its step)
        }
      }
      if (fresh_lane(lane0) < TR_NL) x = bb * mydinv;
    }
    // ---- (6) violated bounds (free set) / multipliers (fixed set): g = H x + c ---------------------
    double pl = 0.0, pt = 0.0;                                // this row of H x: the limb's columns, the trunk's columns
    bool trunk_fixed = false;                                 // workgroup-uniform
    if (fixedm != 0ull) {
      if (dual_tol < 0.0) {                                   // (wave-uniform; most solves never fix a variable)
        const int li = fresh_lane(lane_in);
        dual_tol = 1e-13 * (1.0 + rows3_max(li < n ? fabs((sm + L.o.c)[li]) : 0.0));
      }
      if (ROWS) {                                             // one wavefront: every owner lane reads the whole x
        if (own) xs[dof] = x;
        TR_SYNC();                                                                           // B2
      } else {
        // the products of the row of H (h, read once per solve) with the wavefront's own x: two chains per part.
        // (A padding column's x is an exact zero: any finite H will do.)
        double pl1 = 0.0, pt1 = 0.0;
        if constexpr (FOLD) {
          pl = row_bcast_fma_dot<0, 2, (TR_NL + 1) / 2, false>(pl, x, h);
          pl1 = row_bcast_fma_dot<1, 2, TR_NL / 2, false>(pl1, x, h + 1);
          pt = row_bcast_fma_dot<TR_NL, 2, (TR_NT + 1) / 2, false>(pt, x, h + TR_NL);
          pt1 = row_bcast_fma_dot<TR_NL + 1, 2, TR_NT / 2, false>(pt1, x, h + TR_NL + 1);
        } else {
#pragma unroll
          for (int m = 0; m < TR_NL; m++) {
            const double xm = TR_BCAST(x, m);
            if (m & 1) pl1 = fma(h[m], xm, pl1); else pl = fma(h[m], xm, pl);
          }
#pragma unroll
          for (int u = 0; u < TR_NT; u++) {
            const double xu = TR_BCAST(x, TR_NL + u);
            if (u & 1) pt1 = fma(h[TR_NL + u], xu, pt1); else pt = fma(h[TR_NL + u], xu, pt);
          }
        }
        pl += pl1; pt += pt1;
        // A fixed trunk row (owned by wavefront 0) needs the limb parts of all four wavefronts.  gpart is written
        // here, after B1 of this round, and read after B2; B3 separates that read from the next round's writes.
        // (every wavefront holds the same trunk rows in the same lanes: the vote is workgroup-uniform)
        TR_ROW()
        trunk_fixed = __any(is_trunk && row && self_fixed);
        if (trunk_fixed) {
          if (is_trunk) gpart[wave * TR_MAX_NT + t] = pl;
          TR_SYNC();                                                                         // B2
        }
      }
    }
    PROF_END(pr, PH_MULT);
    PROF_BEGIN(pr);
    int newst = 0;                                            // 0 none, 1 -> lower, 2 -> upper, 3 release
    if (own) {
      if (!self_fixed) {
        if (x < lo - ptol_lo) newst = 1;
        else if (x > hi + ptol_hi) newst = 2;
      } else {
        double g;
        if (ROWS) {
          double g0 = ci, g1 = 0.0;
          // (eight products per trip with all their loads in flight)
          double g2 = 0.0, g3 = 0.0;
          int j = 0;
          for (; j + 7 < n; j += 8) {
            const double h0 = Hrow[j], h1 = Hrow[j + 1], h2 = Hrow[j + 2], h3 = Hrow[j + 3], h4 = Hrow[j + 4], h5 = Hrow[j + 5],
                         h6 = Hrow[j + 6], h7 = Hrow[j + 7];
            const double x0 = xs[j], x1 = xs[j + 1], x2 = xs[j + 2], x3 = xs[j + 3], x4 = xs[j + 4], x5 = xs[j + 5],
                         x6 = xs[j + 6], x7 = xs[j + 7];
            g0 = fma(h0, x0, g0); g1 = fma(h1, x1, g1); g2 = fma(h2, x2, g2); g3 = fma(h3, x3, g3);
            g0 = fma(h4, x4, g0); g1 = fma(h5, x5, g1); g2 = fma(h6, x6, g2); g3 = fma(h7, x7, g3);
          }
          for (; j < n; j++) g0 = fma(Hrow[j], xs[j], g0);
          g = (g0 + g1) + (g2 + g3);
        } else {
          const int lane = fresh_lane(lane0);
          g = ci + (pl + pt);                                 // limb row: its own wavefront holds every column
          if (lane >= TR_NL) {                                // trunk row (wavefront 0): the four limbs' parts
            const double* gp = gpart + (lane - TR_NL);
            g = (ci + pt) + ((gp[0] + gp[TR_MAX_NT]) + (gp[2 * TR_MAX_NT] + gp[3 * TR_MAX_NT]));
          }
        }
        const bool at_lower = (bs.lower >> dof) & 1ull;
        if (at_lower ? g < -dual_tol : g > dual_tol) newst = 3;
      }
    }
    // each violating owner lane sets its dof's bit in the round's set (LDS atomic OR: order-independent)
    if (newst != 0) atomicOr(&vcur[newst - 1], 1ull << dof);
    if (fresh_lane(lane0) == 0 && tbad) atomicOr(&vcur[3], 1ull);
    // Nobody reads xs inside a round of the 4-wavefront form (one wavefront: unless a variable is fixed): a lane
    // without a violation stores its result now, and if the round turns out to be the last one, B3 has already
    // published it -- no trailing store and barrier.  (A violating lane's round is not the last; its store would be
    // overwritten anyway.)
    const bool early = !ROWS || fixedm == 0ull;               // wave- and workgroup-uniform
    if (early && own && newst == 0) xs[dof] = fmin(fmax(x, lo), hi);
    TR_SYNC();                                                                               // B3
    PROF_END(pr, PH_IO);
    const unsigned long long to_lo = vcur[0], to_up = vcur[1], rel = vcur[2];
    if (vcur[3]) return GMR_STATUS_QP_FAILED;
    const unsigned long long all = to_lo | to_up | rel;
    if (all == 0ull) {
      if (!early) {
        if (own) xs[dof] = fmin(fmax(x, lo), hi);
        TR_SYNC();
      }
      return GMR_STATUS_OK;
    }
    const int total = __popcll(all);
    unsigned long long sel = all;                             // block principal pivoting: exchange all
    if (total < ninf_best) { ninf_best = total; pcount = 3; }
    else if (pcount > 0) pcount--;
    else sel = 1ull << (63 - __clzll((long long)all));        // Murty: only the highest violated variable
    bs.lower = (bs.lower & ~(rel & sel)) | (to_lo & sel);
    bs.upper = (bs.upper & ~(rel & sel)) | (to_up & sel);
  }
  return GMR_STATUS_QP_MAXITER;
#undef TR_BCAST
#undef TR_SYNC
#undef TR_DIAG
#undef TR_ROW
}

}  // namespace gmr
