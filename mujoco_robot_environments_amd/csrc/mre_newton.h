// mre_newton.h -- MuJoCo's Newton solver (mj_solPrimal with flg_Newton) for one environment per
// wavefront; compiled into the step kernels built with -DMRE_NEWTON.  Included by
// mre_kernels.hip after mre_solver.h (constraint assembly, row storage).
//
// The reference never sets opt.solver (tasks/rearrangement.py:77-80), so its MuJoCo runs Newton:
// primal problem in qacc,   cost(a) = 1/2 (a - a_smooth)' M (a - a_smooth) + s(J a - aref),
// search direction -H^-1 grad with H = M + J' diag(D_active) J + sum_cone J_c' H_c J_c, exact
// line search along it, termination on scale * improvement or scale * |grad| < tolerance.
//
// Lane mappings.
//   lane = dof (0..38) for generalized vectors, for the rows of H and of its Cholesky factor.
//   lane = contact / lane = scalar row for the constraint update and the line-search terms.
//   H is assembled with the matrix rows in registers (lane j holds H[j][0..38]): one uniform pass
//   over the constraint rows, every lane adds t_j * J_i[c] for the dofs c of the blocks row i
//   touches (J_i[c] by v_readlane: the lane index is a compile-time constant).  H is block
//   structured -- robot 15 x 15, one 6 x 6 block per cube, couplings only where a contact joins two
//   of them -- and the factorisation H = W W' (W upper triangular, eliminated from the last dof to
//   the first: cubes before the robot, like mj_factorM) skips absent blocks by wave-uniform
//   branches, fill-in between blocks included.  The solve W y = g rides along the elimination; the
//   transposed solve W' x = y needs the columns of W, which go through LDS once (packed, 3 KB).
#pragma once

namespace mre {

constexpr int NW_QUAD = 0, NW_SAT = 1, NW_CONE = 4;
constexpr unsigned NW_CPL_ALL_TILES = 0x80u;  // Sm::cpl_robot, above the four cube bits: the launch carries F_NW_ALL_TILES
constexpr int NW_LS_MAX = 20;       // line-search evaluations at most (opt.ls_iterations = 50 in fp64)
constexpr float NW_LS_TOL = 0.01f;  // opt.ls_tolerance
#ifndef NW_LS_REL_VALUE
#define NW_LS_REL_VALUE 1e-5f
#endif
constexpr float NW_LS_REL = NW_LS_REL_VALUE;  // slope reduction at which the fp32 line search stops

MRE_DEV float rdlane(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
MRE_DEV int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
MRE_DEV float unif(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// J_i[dof of this lane]; h = hdr[i] (wave-uniform), lp / lk = cube and local dof of a cube lane
MRE_DEV float nw_Jl(const Sm& s, int i, int h, int l, int lp, int lk) {
  const int rs = h & 0xFF, pa = (h >> 8) & 0xF, pb = (h >> 12) & 0xF;
  float j = 0.f;
  if (l < NRV) {
    if (rs != HDR_NONE) j = s.Jr[rs][l];
  } else if (l < NV) {
    if (pa == lp) j = jpA(s, i)[lk];
    else if (pb == lp) j = jpB(s, i)[lk];
  }
  return j;
}

// (M v)[dof of this lane]; v in LDS
MRE_DEV float nw_mulM(const Sm& s, int l, float mdiag, const float* v) {
  float acc = 0.f;
  if (l < NRV) {
#pragma unroll
    for (int c = 0; c < NRV; c++) acc = fmaf(s.Md[l][c], v[c], acc);
  } else if (l < NV) {
    acc = mdiag * v[l];
  }
  return acc;
}

// One elliptic contact (condim 3) of mj_constraintUpdate: zone, forces, cost, cone Hessian.
// jar -> U = (mu j0, fr j1, fr j2), N = U0, T = |U12|; top zone N >= mu T (no force), bottom
// zone mu N + T <= 0 (quadratic), else the middle zone with cost Dm/2 (N - mu T)^2.
struct NwContact { float f0, f1, f2, cost; int st; };
template <bool HESS>
MRE_DEV NwContact nw_contact(float j0, float j1, float j2, float D0, float D1, float D2, float fr, float mu,
                             float* hc) {
  NwContact o;
  const float U0 = j0 * mu, U1 = j1 * fr, U2 = j2 * fr;
  const float N = U0, T = sqrtf(U1 * U1 + U2 * U2);
  if (N >= mu * T || (T <= 0.f && N >= 0.f)) {
    o.f0 = o.f1 = o.f2 = 0.f; o.cost = 0.f; o.st = NW_SAT;
  } else if (mu * N + T <= 0.f || (T <= 0.f && N < 0.f)) {
    o.f0 = -D0 * j0; o.f1 = -D1 * j1; o.f2 = -D2 * j2;
    o.cost = 0.5f * (D0 * j0 * j0 + D1 * j1 * j1 + D2 * j2 * j2);
    o.st = NW_QUAD;
  } else {
    const float Dm = D0 / fmaxf(mu * mu * (1.f + mu * mu), kMinVal);
    const float NT = N - mu * T, iT = 1.0f / T;
    o.cost = 0.5f * Dm * NT * NT;
    o.f0 = -Dm * NT * mu;
    o.f1 = -o.f0 * iT * U1 * fr;
    o.f2 = -o.f0 * iT * U2 * fr;
    o.st = NW_CONE;
    if (HESS) {
      // d2/djar2: in U coordinates [1, -mu U'/T; ., mu N/T^3 UU' + (mu^2 - mu N/T) I], then
      // pre/post multiplied by diag(mu, fr, fr) and scaled by Dm
      const float a = mu * N * iT * iT * iT, dg = mu * mu - mu * N * iT;
      hc[0] = Dm * mu * mu;
      hc[1] = Dm * mu * fr * (-mu * U1 * iT);
      hc[2] = Dm * mu * fr * (-mu * U2 * iT);
      hc[3] = Dm * fr * fr * (a * U1 * U1 + dg);
      hc[4] = Dm * fr * fr * (a * U1 * U2);
      hc[5] = Dm * fr * fr * (a * U2 * U2 + dg);
    }
  }
  return o;
}

// One pyramidal contact (condim 3) on the same three rows: MuJoCo's four one-sided rows are the edges
// e = j0 +- fr j1, j0 +- fr j2 with one D (assemble_constraints); cost = D/2 sum min(0, e)^2, the force on
// (normal, t1, t2) is minus its gradient, the Hessian D sum_active (1, +-fr, 0)(..)' resp. (1, 0, +-fr)(..)'.
// A contact with any active edge is reported in state NW_CONE (its 3 x 3 Hessian goes through hc like a
// middle-zone elliptic contact's); none active: NW_SAT.
template <bool HESS>
MRE_DEV NwContact nw_pyramid(float j0, float j1, float j2, float D, float fr, float* hc) {
  NwContact o;
  const float e0 = j0 + fr * j1, e1 = j0 - fr * j1, e2 = j0 + fr * j2, e3 = j0 - fr * j2;
  const float a0 = fminf(e0, 0.f), a1 = fminf(e1, 0.f), a2 = fminf(e2, 0.f), a3 = fminf(e3, 0.f);
  o.f0 = -D * ((a0 + a1) + (a2 + a3));
  o.f1 = -D * fr * (a0 - a1);
  o.f2 = -D * fr * (a2 - a3);
  o.cost = 0.5f * D * ((a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3));
  const float n0 = e0 < 0.f ? 1.f : 0.f, n1 = e1 < 0.f ? 1.f : 0.f, n2 = e2 < 0.f ? 1.f : 0.f, n3 = e3 < 0.f ? 1.f : 0.f;
  o.st = (n0 + n1 + n2 + n3) > 0.f ? NW_CONE : NW_SAT;
  if (HESS) {
    hc[0] = D * ((n0 + n1) + (n2 + n3));
    hc[1] = D * fr * (n0 - n1);
    hc[2] = D * fr * (n2 - n3);
    hc[3] = D * fr * fr * (n0 + n1);
    hc[4] = 0.f;
    hc[5] = D * fr * fr * (n2 + n3);
  }
  return o;
}

// mj_constraintUpdate on `jar` (LDS): lane = scalar row and lane = contact.  FULL: forces,
// states and cone Hessians are stored; otherwise only the cost is evaluated.  Returns s(jar).
template <bool FULL, bool PYR>
MRE_DEV float nw_update(Sm& s, int l, int nscalar, int ncon, float mu_scale, const float* jar) {
  constexpr bool pyr = PYR;
  float cost = 0.f;
  if (l < nscalar) {
    const float D = 1.0f / s.efc_R[l], j = jar[l];
    const bool act = l < 7 || j < 0.f;
    if (FULL) {
      const float f = act ? -D * j : 0.f;
      s.frc[l] = f; s.frc_r[l] = f;
      s.rstate[l] = act ? NW_QUAD : NW_SAT;
    }
    cost = act ? 0.5f * D * j * j : 0.f;
  }
  if (l < ncon) {
    const int i = nscalar + 3 * l;
    const float D0 = 1.0f / s.efc_R[i], D1 = 1.0f / s.efc_R[i + 1], D2 = 1.0f / s.efc_R[i + 2];
    const float fr = s.con_fric[l];
    float hc[6];
    const NwContact o = pyr ? nw_pyramid<FULL>(jar[i], jar[i + 1], jar[i + 2], D0, fr, hc)
                            : nw_contact<FULL>(jar[i], jar[i + 1], jar[i + 2], D0, D1, D2, fr, fr * mu_scale, hc);
    cost += o.cost;
    if (FULL) {
      s.frc[i] = o.f0; s.frc[i + 1] = o.f1; s.frc[i + 2] = o.f2;
      const int rs = s.con_rslot[l];
      if (rs != HDR_NONE) { s.frc_r[rs] = o.f0; s.frc_r[rs + 1] = o.f1; s.frc_r[rs + 2] = o.f2; }
      s.rstate[i] = s.rstate[i + 1] = s.rstate[i + 2] = (uint8_t)o.st;
      if (o.st == NW_CONE) {
#pragma unroll
        for (int k = 0; k < 6; k++) s.hc[l][k] = hc[k];
      }
    }
  }
  return wave_sum(cost);
}

// The active set as three lane masks (scalar rows with a force, contacts in the quadratic zone,
// contacts in the cone zone): equal masks = same rows in H.
struct NwMasks { unsigned long long sc, cq, cc; };
MRE_DEV bool operator==(const NwMasks& a, const NwMasks& b) { return a.sc == b.sc && a.cq == b.cq && a.cc == b.cc; }
MRE_DEV NwMasks nw_masks(const Sm& s, int l, int nscalar, int ncon) {
  NwMasks m;
  const int st_s = l < nscalar ? s.rstate[l] : NW_SAT;
  const int st_c = l < ncon ? s.rstate[nscalar + 3 * l] : NW_SAT;
  m.sc = __ballot(st_s == NW_QUAD);
  m.cq = __ballot(st_c == NW_QUAD);
  m.cc = __ballot(st_c == NW_CONE);
  return m;
}

// (J' f)[dof of this lane]: robot lanes run over the robot-row slots, cube lanes over the
// contacts that touch their cube
MRE_DEV float nw_JTf(const Sm& s, int l, int lp, int lk, int nscalar) {
  float acc = 0.f;
  if (l < NRV) {
    const int n = s.nrrow;
    for (int rs = 0; rs < n; rs++) acc = fmaf(s.Jr[rs][l], s.frc_r[rs], acc);
  } else if (l < NV && lp < s.nprops) {
    const int n = s.ccount[lp];
    for (int t = 0; t < n; t++) {
      const int e = s.clist[lp][t], c = e & 0x7F;
      const float* J = (e & 0x80) ? s.JpB[3 * s.con_bslot[c]] : s.JpA[3 * c];
      const float* f = &s.frc[nscalar + 3 * c];
      acc = fmaf(J[lk], f[0], acc);
      acc = fmaf(J[6 + lk], f[1], acc);
      acc = fmaf(J[12 + lk], f[2], acc);
    }
  }
  return acc;
}

// hh[c] += t * J[c] over the dofs c of the blocks the row touches (robot: has_r; cubes pa, pb)
MRE_DEV void nw_rank1(float (&hh)[NV], float t, float J, bool has_r, int pa, int pb) {
  if (has_r) {
#pragma unroll
    for (int c = 0; c < NRV; c++) hh[c] = fmaf(t, rdlane(J, c), hh[c]);
  }
#pragma unroll
  for (int p = 0; p < NPROP; p++) {
    if (pa == p || pb == p) {
#pragma unroll
      for (int k = 0; k < 6; k++) hh[NRV + 6 * p + k] = fmaf(t, rdlane(J, NRV + 6 * p + k), hh[NRV + 6 * p + k]);
    }
  }
}

// One elimination step of H = W W' (columns NV-1 .. 0) with the solve W y = g riding along.
// Lane j holds row j; after the step hh[K] = W[j][K].  nbm = earlier blocks (bit 0 robot, bit
// 1 + p cube p) that column K reaches, fill-in included.
// hh[c] -= u * u[lane c] for c = HI .. LO: the lane values are read eight at a time into scalar registers before the
// eight multiply-adds that use them -- a v_readlane followed at once by the VALU instruction that takes its result
// costs two wait states (an s_nop per column entry in the straightforward loop)
template <int HI, int LO>
MRE_DEV void nw_elim_update(float (&hh)[NV], float u) {
  constexpr int n = HI - LO + 1;
  if constexpr (n > 0) {
#pragma unroll
    for (int g0 = 0; g0 < n; g0 += 8) {
      float t[8];
#pragma unroll
      for (int q = 0; q < 8; q++)
        if (g0 + q < n) t[q] = rdlane(u, HI - g0 - q);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 8; q++)
        if (g0 + q < n) hh[HI - g0 - q] = fmaf(-u, t[q], hh[HI - g0 - q]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int K>
MRE_DEV void nw_elim_col(float (&hh)[NV], float& g, float& y, float& dinv, int l, unsigned nbm) {
  constexpr int blk = K < NRV ? 0 : 1 + (K - NRV) / 6;
  constexpr int b0 = blk == 0 ? 0 : NRV + 6 * (blk - 1);
  const float piv = rdlane(hh[K], K);
  const float d = __builtin_amdgcn_rsqf(fmaxf(piv, 1e-20f));
  const float u = hh[K] * d;
  hh[K] = u;
  const float yk = rdlane(g, K) * d;
  g = fmaf(-u, yk, g);
  y = (l == K) ? yk : y;
  dinv = (l == K) ? d : dinv;
  nw_elim_update<K - 1, b0>(hh, u);
  if constexpr (blk > 0) {
    if constexpr (blk > 3) { if (nbm & (1u << 3)) nw_elim_update<NRV + 17, NRV + 12>(hh, u); }
    if constexpr (blk > 2) { if (nbm & (1u << 2)) nw_elim_update<NRV + 11, NRV + 6>(hh, u); }
    if constexpr (blk > 1) { if (nbm & (1u << 1)) nw_elim_update<NRV + 5, NRV>(hh, u); }
    if (nbm & 1u) nw_elim_update<NRV - 1, 0>(hh, u);
  }
}
template <int K, int KEND>
MRE_DEV void nw_elim_range(float (&hh)[NV], float& g, float& y, float& dinv, int l, unsigned nbm) {
  nw_elim_col<K>(hh, g, y, dinv, l, nbm);
  if constexpr (K > KEND) nw_elim_range<K - 1, KEND>(hh, g, y, dinv, l, nbm);
}

struct NwPoint { float alpha, cost, d1, d2; };

// Per-cube contact lists and the block coupling of the Hessian (lane 0, after the assembly has
// fixed the kept contacts and their robot slots).  A phase of its own: the row assembly is at the
// edge of its register budget.
// flags: the launch's StepFlags; F_NW_ALL_TILES rides to nw_direction in a spare bit of the robot mask it reads anyway.
MRE_PHASE_FN void nw_build_lists(Sm& s, int l, unsigned flags) {
  // lane = contact; a cube's list is the ascending run of the contacts that touch it (ballot prefix counts)
  const int kept = s.ncon;
  const bool on = l < kept;
  const int cb1 = on ? s.con_b1[l] : 0, cb2 = on ? s.con_b2[l] : 0;
  int pa = -1, pb = -1;
  if (cb1 >= NRB) pa = cb1 - NRB;
  if (cb2 >= NRB) { if (pa < 0) pa = cb2 - NRB; else pb = cb2 - NRB; }
  const unsigned long long lt = (1ull << l) - 1ull;
  const bool rob = on && pa >= 0 && s.con_rslot[on ? l : 0] != HDR_NONE;
  unsigned cr = 0u, cc = 0u;
#pragma unroll
  for (int p = 0; p < NPROP; p++) {
    const bool mine = on && (pa == p || pb == p);
    const unsigned long long m = __ballot(mine);
    if (mine) s.clist[p][__popcll(m & lt)] = (uint8_t)(pb == p ? (l | 0x80) : l);
    if (l == 0) s.ccount[p] = (uint8_t)__popcll(m);
    if (__ballot(rob && pa == p) != 0ull) cr |= 1u << p;
  }
  const int pairbit = (on && pb >= 0) ? cube_pair_bit(pa, pb) : -1;
#pragma unroll
  for (int b = 0; b < 6; b++)
    if (__ballot(pairbit == b) != 0ull) cc |= 1u << b;
  if ((flags & F_NW_ALL_TILES) != 0u) cr |= NW_CPL_ALL_TILES;
  if (l == 0) { s.cpl_robot = (uint8_t)cr; s.cpl_cubes = (uint8_t)cc; }
  // lane = row: where the row's Jacobian words of every cube live (read by the matrix-core pass of nw_direction)
  const int nscalar = 7 + s.nl;
  const unsigned zoff = (unsigned)offsetof(Sm, zrow);
  for (int i = l; i < s.nefc; i += 64) {
    const int h = s.hdr[i], ra = (h >> 8) & 0xF, rb = (h >> 12) & 0xF;
    const int crow = i - nscalar;   // contact row (scalar rows carry no cube part: ra = rb = 0xF)
    const unsigned offA = crow >= 0 ? (unsigned)offsetof(Sm, JpA) + 24u * (unsigned)crow : zoff;
    const unsigned offB = (crow >= 0 && rb != 0xF)
                              ? (unsigned)offsetof(Sm, JpB) + 24u * (unsigned)(3 * s.con_bslot[crow / 3] + crow % 3) : zoff;
#pragma unroll
    for (int cb = 0; cb < NPROP; cb++) s.jdesc[i][cb] = (uint16_t)(ra == cb ? offA : (rb == cb ? offB : zoff));
  }
  MRE_SYNC();
}

// Per-lane constants of the solver phases
struct NwLane {
  int lp, lk;       // cube and local dof of a cube lane (lp = -1: not a cube lane)
  bool lact;        // this lane owns an active dof
  float mdiag;      // cube lanes: diagonal entry of M
  float mu_scale;   // mu = friction * sqrt(R1 / R0) = friction / sqrt(impratio)
  float scale;      // 1 / (meaninertia * nv)
};
MRE_DEV NwLane nw_lane(ModelP M, const Sm& s, int l) {
  NwLane c;
  c.lp = (l >= NRV && l < NV) ? (l - NRV) / 6 : -1;
  c.lk = (l >= NRV && l < NV) ? (l - NRV) % 6 : 0;
  c.lact = l < NRV || (c.lp >= 0 && c.lp < s.nprops);
  c.mdiag = c.lp >= 0 ? (c.lk < 3 ? s.prop_mass[c.lp] : s.prop_inertia[c.lp][c.lk - 3]) : 0.f;
  c.mu_scale = __builtin_amdgcn_rsqf(fmaxf(M->opt_rec.impratio, kMinVal));
  float msum = M->opt_rec.M0_diag_robot_sum;
  for (int p = 0; p < s.nprops; p++)
    msum += 3.f * s.prop_mass[p] + s.prop_inertia[p][0] + s.prop_inertia[p][1] + s.prop_inertia[p][2];
  c.scale = 1.0f / msum;
  return c;
}

// constraint update on s.jar, qfrc_con = J' f, gradient; returns the primal cost.
// In: s.qacc (current iterate), s.nw_Ma.  Out: s.frc, s.rstate, s.hc, s.qfrc_con, s.nw_grad.
template <bool PYR>
MRE_DEV float nw_update_gradient(Sm& s, int l, const NwLane& c, int nscalar, int ncon) {
  const float sc = nw_update<true, PYR>(s, l, nscalar, ncon, c.mu_scale, s.jar);
  MRE_SYNC();
  const float qc = nw_JTf(s, l, c.lp, c.lk, nscalar);
  const bool on = l < NV && c.lact;
  const float fs = on ? s.qfrc_smooth[l] : 0.f, as = on ? s.qacc_smooth[l] : 0.f;
  const float qa = on ? s.qacc[l] : 0.f, Ma = on ? s.nw_Ma[l] : 0.f;
  if (l < NVP) {
    s.qfrc_con[l] = on ? qc : 0.f;
    s.nw_grad[l] = on ? Ma - fs - qc : 0.f;
  }
  const float cost = sc + wave_sum(0.5f * (Ma - fs) * (qa - as));
  MRE_SYNC();
  return cost;
}

// Phase 1: dense robot M, warm start (the cheaper of qacc_warmstart and qacc_smooth in primal
// cost), first constraint update and gradient.  Returns the cost.
template <bool PYR>
MRE_DEV float nw_setup_impl(ModelP M, Sm& s, int l) {
  MRE_DBG_T0();
  const NwLane c = nw_lane(M, s, l);
  const int nefc = s.nefc, ncon = s.ncon, nscalar = 7 + s.nl;
  // (the dense robot block cannot be written by crb_mass_matrix: the narrow phase's per-lane clip buffers run over
  //  this part of Sm between the two)
  for (int e = l; e < NRV * MD_LD; e += 64) (&s.Md[0][0])[e] = 0.f;
  MRE_SYNC();
  for (int e = l; e < NMR; e += 64) {
    const int i = M->M_i[e], j = M->M_j[e];
    const float v = s.qM[e];
    s.Md[i][j] = v; s.Md[j][i] = v;
  }
  MRE_SYNC();
  MRE_DBG_STAMP(10, 0);
  const bool on = l < NV && c.lact;
  const float fs = on ? s.qfrc_smooth[l] : 0.f, as = on ? s.qacc_smooth[l] : 0.f;
  float qa = on ? s.qacc[l] : 0.f;
  float Ma = on ? nw_mulM(s, l, c.mdiag, s.qacc) : 0.f;
  for (int i = l; i < nefc; i += 64) {
    const float aref = s.efc_aref[i];
    float d1, d2;
    row_dot2(s, i, s.qacc, s.qacc_smooth, d1, d2);
    s.jar[i] = d1 - aref;
    s.jv[i] = d2 - aref;
  }
  MRE_SYNC();
  MRE_DBG_STAMP(10, 1);
  const float gauss = wave_sum(0.5f * (Ma - fs) * (qa - as));
  const float cost_ws = gauss + nw_update<false, PYR>(s, l, nscalar, ncon, c.mu_scale, s.jar);
  const float cost_sm = nw_update<false, PYR>(s, l, nscalar, ncon, c.mu_scale, s.jv);
  const bool smooth_wins = cost_ws > cost_sm || !(cost_ws == cost_ws);
#if defined(MRE_PHASE_STAMPS) && MRE_PHASE_STAMPS == 11
  // diagnostic build 11 counts: set-up calls of the launch and those in which qacc_smooth beat the warm start
  if (threadIdx.x == 0) { dbg_acc[0] += 1ull << 4; dbg_acc[1] += (unsigned long long)smooth_wins << 4; }
#endif
  if (smooth_wins) {
    qa = as; Ma = fs;  // M qacc_smooth = qfrc_smooth
    for (int i = l; i < nefc; i += 64) s.jar[i] = s.jv[i];
  }
  if (l < NVP) { s.qacc[l] = qa; s.nw_Ma[l] = Ma; }
  MRE_SYNC();
  MRE_DBG_STAMP(10, 2);
  const float cost = nw_update_gradient<PYR>(s, l, c, nscalar, ncon);
  MRE_DBG_STAMP(10, 3);
  return cost;
}
MRE_PHASE_FN float nw_setup(ModelP M, Sm& s, int l) { return nw_setup_impl<false>(M, s, l); }
MRE_PHASE_FN float nw_setup_pyramidal(ModelP M, Sm& s, int l) { return nw_setup_impl<true>(M, s, l); }

// Phase 2: search = -H^-1 grad.  H = M + J' D J (+ cone Hessians) with its rows in registers,
// block-sparse factorisation H = W W', both triangular solves.
// Bit NW_CPL_ALL_TILES of s.cpl_robot (F_NW_ALL_TILES): also form and move the cross tiles that the contact set leaves zero.
MRE_PHASE_FN void nw_direction(ModelP M, Sm& s, int l) {
  MRE_DBG_T0();
  const NwLane c = nw_lane(M, s, l);
  const int nefc = s.nefc, nscalar = 7 + s.nl, nprops = s.nprops;
  const int lp = c.lp, lk = c.lk;
  // Which cross tiles a row of this step can reach.  A row feeds a cross tile only if it has both parts: equality and
  // limit rows are robot-only, cube-table contacts cube-only, so c10 / c20 (cubes 0-1 / 2-3 x robot) take a kept
  // contact that joins the robot to a cube of the group (cpl_robot) and c21 one that joins a cube of {0, 1} to one of
  // {2, 3} (cpl_cubes) -- the masks that already tell the elimination which blocks fill in.  A tile that is not
  // formed leaves its part of hh as it was initialised: these are off-diagonal blocks, set from the literal 0.f below
  // (Md enters the robot x robot block only, which c00 always serves), and a formed tile without such a row is +0.0 in
  // every word that is read (accumulators start at +0.0 and only take products with a zero word of the row), so
  // "+= +0.0" on +0.0 and no addition at all leave the same bits.
  bool t10, t20, t21;
  {
    const unsigned cr = (unsigned)uni((int)s.cpl_robot), cq = (unsigned)uni((int)s.cpl_cubes);
    constexpr unsigned across = (1u << cube_pair_bit(0, 2)) | (1u << cube_pair_bit(0, 3)) | (1u << cube_pair_bit(1, 2)) |
                                (1u << cube_pair_bit(1, 3));
    const bool all_tiles = (cr & NW_CPL_ALL_TILES) != 0u;
    t10 = all_tiles || (cr & 0x3u) != 0u;
    t20 = all_tiles || (cr & 0xCu) != 0u;
    t21 = all_tiles || (cq & across) != 0u;
  }
#if defined(MRE_PHASE_STAMPS) && MRE_PHASE_STAMPS == 9
  // diagnostic build 9 counts, it does not time: direction calls of the launch, and those that skipped c10 / c20 / c21
  if (threadIdx.x == 0) {
    dbg_acc[0] += 1ull << 4; dbg_acc[1] += (unsigned long long)!t10 << 4;
    dbg_acc[2] += (unsigned long long)!t20 << 4; dbg_acc[3] += (unsigned long long)!t21 << 4;
  }
#endif
  float hh[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) {
    float v = 0.f;
    if (k < NRV) { if (l < NRV) v = s.Md[l][k]; }
    else if (l == k) v = c.lact ? c.mdiag : 1.0f;
    hh[k] = v;
  }
  // ---- J' diag(D) J over the rows in the quadratic state: a genuine contraction (39 x nefc times nefc x 39),
  // done on the matrix cores.  The 39 dofs are laid out in three 16-wide tiles (0: robot dofs 0..14, 1: cubes 0
  // and 1, 2: cubes 2 and 3; 6 dofs each, the rest padding); v_mfma_f32_16x16x4_f32 consumes four rows per
  // issue: operand lane 16 k + m holds row r0 + k at tile dof m (A = J D, B = J), and the six tiles of the lower
  // triangle accumulate in 24 registers.  Per chunk of four rows a lane fetches its row's header, state and 1 / R
  // and ONE Jacobian word per tile -- no per-row branches, no cross-lane traffic.  Rows in any other state enter with D = 0.
  MRE_DBG_STAMP(4, 0);
#if defined(MRE_PHASE_STAMPS) && MRE_PHASE_STAMPS == 5
  {  // diagnostic build 5, words 2 and 3: rows in the cone / quadratic state over the direction calls of the launch
    int nc_ = 0, nq_ = 0;
    for (int r0 = 0; r0 < nefc; r0 += 64) {
      const int st_ = r0 + l < nefc ? (int)s.rstate[r0 + l] : NW_SAT;
      nc_ += __popcll(__ballot(st_ == NW_CONE)); nq_ += __popcll(__ballot(st_ == NW_QUAD));
    }
    if (threadIdx.x == 0) { dbg_acc[2] += (unsigned long long)nc_ << 4; dbg_acc[3] += (unsigned long long)nq_ << 4; }
  }
#endif
  typedef float v4f __attribute__((ext_vector_type(4)));
  v4f c00 = {0.f, 0.f, 0.f, 0.f}, c10 = c00, c11 = c00, c20 = c00, c21 = c00, c22 = c00;
  {
    const int g = l >> 4, m16 = l & 15;
    // Per chunk of four rows a lane reads its row's descriptor (jdesc: one 8-byte word), header, state and R one
    // chunk ahead, then ONE Jacobian word per tile at descriptor offset + lane offset: no compares, no per-row
    // branches.  Lanes past a tile's dofs (m16 = 15; m16 >= 12 in the cube tiles) read whatever lies there: they
    // only feed accumulator rows / columns that are never read.  Rows outside the quadratic state enter with A = 0.
    const char* const sb = reinterpret_cast<const char*>(&s);
    const unsigned zoff = (unsigned)offsetof(Sm, zrow), jr0 = (unsigned)offsetof(Sm, Jr);
    const unsigned sh = m16 < 12 ? 16u * (unsigned)(m16 / 6) : 0u;   // which half of a descriptor dword
    const unsigned lo = 4u * (unsigned)(m16 % 6), lr = 4u * (unsigned)m16;
    auto ldw = [&](unsigned off) { return *reinterpret_cast<const float*>(sb + off); };
    auto meta = [&](int r0, int& ii, int& st, int& h, float& R, uint2& d) {
      const int i = r0 + g;
      ii = i < nefc ? i : 0;
      st = i < nefc ? (int)s.rstate[ii] : NW_SAT;
      h = s.hdr[ii];
      R = s.efc_R[ii];
      d = *reinterpret_cast<const uint2*>(&s.jdesc[ii][0]);
    };
    // the row's words at this lane's dof of the three tiles
    auto gather = [&](int h, uint2 d, float& w0, float& w1, float& w2) {
      const int rs = h & 0xFF;
      w0 = ldw((rs != HDR_NONE ? jr0 + 60u * (unsigned)rs : zoff) + lr);
      w1 = ldw(((d.x >> sh) & 0xFFFFu) + lo);
      w2 = nprops > 2 ? ldw(((d.y >> sh) & 0xFFFFu) + lo) : 0.f;
    };
    static_assert(sizeof(s.Jr[0]) == 60 && sizeof(s.JpA[0]) == 24 && sizeof(s.JpB[0]) == 24, "row strides of the gathers");
    // one chunk on the metadata `cur`; the metadata of the following chunk goes to `nxt`.  The loop calls it with
    // two sets in turn, so no registers are shuffled between chunks.
    struct Meta { int ii, st, h; float R; uint2 d; };
    // cross (compile time): the step has a cross tile.  The loop exists twice, so that the common step -- none --
    // runs its three diagonal MFMAs with no test per chunk (tests inside the chunk cost more than the MFMAs they
    // save: profiles/NOTES.md, round 5); with a cross tile the three flags pick per tile.
    auto chunk = [&](auto cross, const Meta& cur, Meta& nxt, int r0) {
      const int ii = cur.ii, h = cur.h, st = cur.st;
      const uint2 d = cur.d;
      const bool quad = st == NW_QUAD, cone = st == NW_CONE;
      const float D = quad ? __builtin_amdgcn_rcpf(cur.R) : 0.f;   // (1 ulp; the IEEE division is 12 instructions)
      if (r0 + 4 < nefc) meta(r0 + 4, nxt.ii, nxt.st, nxt.h, nxt.R, nxt.d);
      float v0, v1, v2, a0, a1, a2;
      if (__any(cone)) {
        // a contact in the middle zone enters with its 3 x 3 Hessian: row k of the contact contributes
        // (sum_m Hc[k][m] J_m)' J_k, so the A operand of such a lane is the Hc-weighted mix of the contact's three
        // rows (consecutive rows, slots and parts) at its dof; the other lanes of the chunk read their own row
        const int cr = ii - nscalar;
        const int k = cone ? cr % 3 : 0;
        const int i0 = ii - k, i1 = cone ? i0 + 1 : ii, i2 = cone ? i0 + 2 : ii;
        float x0, x1, x2, y0, y1, y2, z0, z1, z2;
        gather(s.hdr[i0], *reinterpret_cast<const uint2*>(&s.jdesc[i0][0]), x0, x1, x2);
        gather(s.hdr[i1], *reinterpret_cast<const uint2*>(&s.jdesc[i1][0]), y0, y1, y2);
        gather(s.hdr[i2], *reinterpret_cast<const uint2*>(&s.jdesc[i2][0]), z0, z1, z2);
        const float* hcp = s.hc[cone ? cr / 3 : 0];
        const float H0 = k == 0 ? hcp[0] : (k == 1 ? hcp[1] : hcp[2]);
        const float H1 = k == 0 ? hcp[1] : (k == 1 ? hcp[3] : hcp[4]);
        const float H2 = k == 0 ? hcp[2] : (k == 1 ? hcp[4] : hcp[5]);
        v0 = k == 0 ? x0 : (k == 1 ? y0 : z0);
        v1 = k == 0 ? x1 : (k == 1 ? y1 : z1);
        v2 = k == 0 ? x2 : (k == 1 ? y2 : z2);
        a0 = cone ? H0 * x0 + H1 * y0 + H2 * z0 : v0 * D;
        a1 = cone ? H0 * x1 + H1 * y1 + H2 * z1 : v1 * D;
        a2 = cone ? H0 * x2 + H1 * y2 + H2 * z2 : v2 * D;
      } else {
        gather(h, d, v0, v1, v2);
        a0 = v0 * D; a1 = v1 * D; a2 = v2 * D;
      }
      c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, v0, c00, 0, 0, 0);
      if constexpr (decltype(cross)::value) { if (t10) c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, v0, c10, 0, 0, 0); }
      c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, v1, c11, 0, 0, 0);
      if (nprops > 2) {   // (wave-uniform: cubes 2 and 3 exist)
        if constexpr (decltype(cross)::value) {
          if (t20) c20 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, v0, c20, 0, 0, 0);
          if (t21) c21 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, v1, c21, 0, 0, 0);
        }
        c22 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, v2, c22, 0, 0, 0);
      }
    };
    Meta mA, mB;
    meta(0, mA.ii, mA.st, mA.h, mA.R, mA.d);
    mB = mA;
    using NwYes = std::integral_constant<bool, true>;
    using NwNo = std::integral_constant<bool, false>;
    if (t10 || t20 || t21) {
      for (int r0 = 0; r0 < nefc; r0 += 8) {
        chunk(NwYes{}, mA, mB, r0);
        if (r0 + 4 < nefc) chunk(NwYes{}, mB, mA, r0 + 4);
      }
    } else {
      for (int r0 = 0; r0 < nefc; r0 += 8) {
        chunk(NwNo{}, mA, mB, r0);
        if (r0 + 4 < nefc) chunk(NwNo{}, mB, mA, r0 + 4);
      }
    }
    MRE_DBG_STAMP(4, 1);
    // Tiles -> rows: lane j needs row j of H.  One tile at a time through LDS (the factor's home, unused until
    // the elimination is over): the accumulator of lane 16 q + n holds C[4 q + v][n], v = 0..3.  The lanes that
    // own the tile's row dofs read a row, and for an off-diagonal tile the lanes that own its column dofs
    // read a column (H is symmetric).
    float* T = s.W;
    constexpr int TS = 17;
    // this lane's tile and index in it (lane = dof)
    const int mytile = l < NRV ? 0 : (l < NRV + 12 ? 1 : (l < NV ? 2 : -1));
    const int mym = l < NRV ? l : (l < NRV + 12 ? l - NRV : l - NRV - 12);
    auto spill = [&](const v4f& cv, int off) {
#pragma unroll
      for (int v = 0; v < 4; v++) T[off + (4 * g + v) * TS + m16] = cv[v];
    };
    // (TI, TJ): tile row / column block; BI, BJ: first hh index of the blocks; NI, NJ: dofs in them; two
    // tiles share a round trip (the factor's LDS holds two padded 16 x 17 tiles)
#define NW_TILE(OFF, TI, TJ, BI, NI, BJ, NJ)                                                   \
    if (mytile == TI) {                                                                        \
      _Pragma("unroll") for (int n = 0; n < NJ; n++) hh[BJ + n] += T[OFF + mym * TS + n];      \
    }                                                                                          \
    if (TI != TJ && mytile == TJ) {                                                            \
      _Pragma("unroll") for (int q = 0; q < NI; q++) hh[BI + q] += T[OFF + q * TS + mym];      \
    }
    constexpr int T2 = 16 * TS;
    static_assert(2 * T2 <= NV * (NV + 1) / 2, "two tiles fit the factor's storage");
    // (every word of hh takes its sum from ONE tile, so which tiles share a trip changes no bit)
    if (t10 || t20 || t21) {
      spill(c00, 0);
      if (t10) spill(c10, T2);
      MRE_SYNC();
      NW_TILE(0, 0, 0, 0, NRV, 0, NRV)
      if (nprops > 0 && t10) { NW_TILE(T2, 1, 0, NRV, 12, 0, NRV) }
      MRE_SYNC();
      if (nprops > 0) {
        spill(c11, 0);
        if (t20) spill(c20, T2);
        MRE_SYNC();
        NW_TILE(0, 1, 1, NRV, 12, NRV, 12)
        if (nprops > 2 && t20) { NW_TILE(T2, 2, 0, NRV + 12, 12, 0, NRV) }
        MRE_SYNC();
      }
      if (nprops > 2) {
        if (t21) spill(c21, 0);
        spill(c22, T2);
        MRE_SYNC();
        if (t21) { NW_TILE(0, 2, 1, NRV + 12, 12, NRV, 12) }
        NW_TILE(T2, 2, 2, NRV + 12, 12, NRV + 12, 12)
        MRE_SYNC();
      }
    } else {
      // no cross tile: the three diagonal tiles take two trips (one for an env of at most two cubes) instead of three
      spill(c00, 0);
      if (nprops > 0) spill(c11, T2);
      MRE_SYNC();
      NW_TILE(0, 0, 0, 0, NRV, 0, NRV)
      if (nprops > 0) { NW_TILE(T2, 1, 1, NRV, 12, NRV, 12) }
      MRE_SYNC();
      if (nprops > 2) {
        spill(c22, 0);
        MRE_SYNC();
        NW_TILE(0, 2, 2, NRV + 12, 12, NRV + 12, 12)
        MRE_SYNC();
      }
    }
#undef NW_TILE
  }
  MRE_DBG_STAMP(4, 2);
  // symbolic elimination over the blocks (node 0 robot, node 1 + p cube p), cubes last to first
  unsigned adj[5];
  {
    const unsigned cr = s.cpl_robot, cq = s.cpl_cubes;
    adj[0] = 0u;
#pragma unroll
    for (int p = 0; p < NPROP; p++) {
      unsigned a = (cr >> p) & 1u;  // robot
#pragma unroll
      for (int q = 0; q < NPROP; q++)
        if (q != p && ((cq >> cube_pair_bit(p, q)) & 1u)) a |= 1u << (1 + q);
      adj[1 + p] = a;
    }
#pragma unroll
    for (int a = 4; a >= 1; a--) {
      const unsigned nb = adj[a] & ((1u << a) - 1u);  // earlier blocks reached by block a
#pragma unroll
      for (int b = 1; b < 4; b++)
        if (b < a && ((nb >> b) & 1u)) adj[b] |= nb & ~(1u << b);
    }
#pragma unroll
    for (int a = 1; a < 5; a++) adj[a] = (unsigned)uni((int)adj[a]);
  }
  float g = l < NVP ? s.nw_grad[l] : 0.f, y = 0.f, dinv = 1.0f;
  if (nprops > 3) nw_elim_range<NRV + 23, NRV + 18>(hh, g, y, dinv, l, adj[4] & 0xFu);
  if (nprops > 2) nw_elim_range<NRV + 17, NRV + 12>(hh, g, y, dinv, l, adj[3] & 0x7u);
  if (nprops > 1) nw_elim_range<NRV + 11, NRV + 6>(hh, g, y, dinv, l, adj[2] & 0x3u);
  if (nprops > 0) nw_elim_range<NRV + 5, NRV>(hh, g, y, dinv, l, adj[1] & 0x1u);
  nw_elim_range<NRV - 1, 0>(hh, g, y, dinv, l, 0u);
  MRE_DBG_STAMP(4, 3);
  // ---- W' x = y: columns of W through LDS (packed by columns: (j, k), j <= k at k(k+1)/2 + j)
#pragma unroll
  for (int k = 0; k < NV; k++)
    if (l <= k) s.W[k * (k + 1) / 2 + l] = hh[k];
  MRE_SYNC();
  {
    // column l of W (rows j < l) into the registers the H rows just left: 38 independent LDS reads, then
    // the dependent chain y_l -= W[j][l] x_j runs on registers with compile-time lanes
    const int base = l < NV ? l * (l + 1) / 2 : 0;
    const int nva = NRV + 6 * nprops;  // inactive cube blocks: x = 0
#pragma unroll
    for (int j = 0; j < NV - 1; j++) hh[j] = (j < l && l < nva) ? s.W[base + j] : 0.f;
#pragma unroll
    for (int j = 0; j < NV - 1; j++) {
      const float xj = rdlane(y * dinv, j);
      y = fmaf(-hh[j], xj, y);
    }
  }
  const float x = (l < NV && c.lact) ? y * dinv : 0.f;
  if (l < NVP) s.nw_search[l] = -x;
  // Newton decrement grad' H^-1 grad: the cost decrease the quadratic model predicts is half of it
  const float dec = wave_sum((l < NVP ? s.nw_grad[l] : 0.f) * x);
  if (l == 0) s.scratch[2] = dec;
  MRE_SYNC();
  MRE_DBG_STAMP(4, 3);
}

// Phase 2': the same direction from the factor of the last nw_direction call (still in s.W), for a
// gradient whose active set did not change -- MuJoCo's Newton likewise keeps its Cholesky factor
// while the constraint states stand.  Both triangular solves read W from LDS: W y = g by columns
// (for column k the lanes j < k read consecutive words), W' x = y as in nw_direction.
MRE_PHASE_FN void nw_direction_reuse(ModelP M, Sm& s, int l) {
  const NwLane c = nw_lane(M, s, l);
  const int nva = NRV + 6 * s.nprops;
  const bool on = l < NV && c.lact;
  const float gin = on ? s.nw_grad[l] : 0.f;
  float g = gin;
  const float dinv = on ? 1.0f / s.W[l * (l + 1) / 2 + l] : 1.0f;
  float y = 0.f;
  for (int k = nva - 1; k >= 0; k--) {
    const float yk = rdlane(g * dinv, k);
    const float w = (l < k) ? s.W[k * (k + 1) / 2 + l] : 0.f;
    g = fmaf(-w, yk, g);
    y = (l == k) ? yk : y;
  }
  const int base = l < NV ? l * (l + 1) / 2 : 0;
  for (int j = 0; j < nva; j++) {
    const float cw = (j < l && l < NV) ? s.W[base + j] : 0.f;
    const float xj = rdlane(y * dinv, j);
    y = fmaf(-cw, xj, y);
  }
  const float x = on ? y * dinv : 0.f;
  if (l < NVP) s.nw_search[l] = -x;
  const float dec = wave_sum(gin * x);
  if (l == 0) s.scratch[2] = dec;
  MRE_SYNC();
}

// Phase 3: exact line search along s.nw_search (PrimalSearch), move, constraint update, gradient.
// Returns the new cost; s.scratch[0] = step (0 when no step was possible), s.scratch[1] = |grad|.
template <bool PYR>
MRE_DEV float nw_search_move_impl(ModelP M, Sm& s, int l) {
  MRE_DBG_T0();
  const NwLane c = nw_lane(M, s, l);
  const int nefc = s.nefc, ncon = s.ncon, nscalar = 7 + s.nl;
  const float tol = M->opt_rec.tolerance, mu_scale = c.mu_scale;
  const bool on = l < NV && c.lact;
  const float fs = on ? s.qfrc_smooth[l] : 0.f, as = on ? s.qacc_smooth[l] : 0.f;
  float qa = on ? s.qacc[l] : 0.f, Ma = on ? s.nw_Ma[l] : 0.f;
  const float sv = on ? s.nw_search[l] : 0.f;
  const float Mv = on ? nw_mulM(s, l, c.mdiag, s.nw_search) : 0.f;
  for (int i = l; i < nefc; i += 64) s.jv[i] = row_dot(s, i, s.nw_search);
  MRE_SYNC();
  MRE_DBG_STAMP(7, 0);
  const float snorm = sqrtf(wave_sum(sv * sv));
  float alpha = 0.f;
#if defined(MRE_PHASE_STAMPS) && MRE_PHASE_STAMPS == 7
  int dbg_nev = 0;   // diagnostic build 7: evaluations per tick go to the set's fourth word
#endif
  if (snorm >= kMinVal) {
    const float gtol_abs = tol * NW_LS_TOL * snorm / c.scale;
    float g0 = 0.5f * (Ma - fs) * (qa - as), g1 = sv * (Ma - fs), g2 = 0.5f * sv * Mv;
    wave_sum3(g0, g1, g2);
    // per-lane terms: one scalar row and one contact
    float sq0 = 0.f, sq1 = 0.f, sq2 = 0.f, sj = 0.f, svv = 0.f;
    const bool s_on = l < nscalar, s_eq = l < 7;
    if (s_on) {
      const float D = 1.0f / s.efc_R[l];
      sj = s.jar[l]; svv = s.jv[l];
      sq0 = 0.5f * D * sj * sj; sq1 = D * sj * svv; sq2 = 0.5f * D * svv * svv;
    }
    float cq0 = 0.f, cq1 = 0.f, cq2 = 0.f, U0 = 0.f, V0 = 0.f, UU = 0.f, UV = 0.f, VV = 0.f, Dm = 0.f, mu = 0.f;
    const bool c_on = l < ncon;
    constexpr bool pyr = PYR;
    // pyramidal cones: the four edges' jar and J*search (nw_pyramid), one D
    float pe0 = 0.f, pe1 = 0.f, pe2 = 0.f, pe3 = 0.f, pv0 = 0.f, pv1 = 0.f, pv2 = 0.f, pv3 = 0.f, pD = 0.f;
    if (c_on && pyr) {
      const int i = nscalar + 3 * l;
      const float fr = s.con_fric[l];
      const float j0 = s.jar[i], j1 = fr * s.jar[i + 1], j2 = fr * s.jar[i + 2];
      const float v0 = s.jv[i], v1 = fr * s.jv[i + 1], v2 = fr * s.jv[i + 2];
      pe0 = j0 + j1; pe1 = j0 - j1; pe2 = j0 + j2; pe3 = j0 - j2;
      pv0 = v0 + v1; pv1 = v0 - v1; pv2 = v0 + v2; pv3 = v0 - v2;
      pD = 1.0f / s.efc_R[i];
    }
    if (c_on && !pyr) {
      const int i = nscalar + 3 * l;
      const float fr = s.con_fric[l];
      mu = fr * mu_scale;
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const float D = 1.0f / s.efc_R[i + r], j = s.jar[i + r], v = s.jv[i + r];
        cq0 += 0.5f * D * j * j; cq1 += D * j * v; cq2 += 0.5f * D * v * v;
      }
      const float U1 = s.jar[i + 1] * fr, U2 = s.jar[i + 2] * fr, V1 = s.jv[i + 1] * fr, V2 = s.jv[i + 2] * fr;
      U0 = s.jar[i] * mu; V0 = s.jv[i] * mu;
      UU = U1 * U1 + U2 * U2; UV = U1 * V1 + U2 * V2; VV = V1 * V1 + V2 * V2;
      Dm = (1.0f / s.efc_R[i]) / fmaxf(mu * mu * (1.f + mu * mu), kMinVal);
    }
#if defined(MRE_PHASE_STAMPS) && MRE_PHASE_STAMPS == 7
#define NW_DBG_EVAL() dbg_nev++
#else
#define NW_DBG_EVAL() do {} while (0)
#endif
    auto eval = [&](float a) {  // PrimalEval
      NW_DBG_EVAL();
      float q0 = 0.f, q1 = 0.f, q2 = 0.f, ec = 0.f, e1 = 0.f, e2 = 0.f;
      if (s_on && (s_eq || sj + a * svv < 0.f)) { q0 = sq0; q1 = sq1; q2 = sq2; }
      if (c_on && pyr) {
        const float x0 = fminf(pe0 + a * pv0, 0.f), x1 = fminf(pe1 + a * pv1, 0.f);
        const float x2 = fminf(pe2 + a * pv2, 0.f), x3 = fminf(pe3 + a * pv3, 0.f);
        ec = 0.5f * pD * ((x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3));
        e1 = pD * ((x0 * pv0 + x1 * pv1) + (x2 * pv2 + x3 * pv3));
        e2 = pD * (((x0 < 0.f ? pv0 * pv0 : 0.f) + (x1 < 0.f ? pv1 * pv1 : 0.f)) +
                   ((x2 < 0.f ? pv2 * pv2 : 0.f) + (x3 < 0.f ? pv3 * pv3 : 0.f)));
      }
      if (c_on && !pyr) {
        const float N = U0 + a * V0, Tsqr = UU + a * (2.f * UV + a * VV);
        bool quad = false;
        if (Tsqr <= 0.f) {
          quad = N < 0.f;
        } else {
          const float T = sqrtf(Tsqr);
          if (N >= mu * T) {
          } else if (mu * N + T <= 0.f) {
            quad = true;
          } else {
            const float iT = 1.0f / T;
            const float b = UV + a * VV;
            const float N1 = V0, T1 = b * iT, T2 = VV * iT - b * b * iT * iT * iT;
            const float NT = N - mu * T, w = N1 - mu * T1;
            ec = 0.5f * Dm * NT * NT;
            e1 = Dm * NT * w;
            e2 = Dm * (w * w - NT * mu * T2);
          }
        }
        if (quad) { q0 += cq0; q1 += cq1; q2 += cq2; }
      }
      NwPoint p;
      p.alpha = a;
      float s0 = ec + q0 + a * (q1 + a * q2), s1 = e1 + q1 + 2.f * a * q2, s2 = e2 + 2.f * q2;
      wave_sum3(s0, s1, s2);
      p.cost = s0 + g0 + a * (g1 + a * g2);
      p.d1 = s1 + g1 + 2.f * a * g2;
      p.d2 = s2 + 2.f * g2;
      return p;
    };
    const NwPoint p0 = eval(0.f);
    if (p0.d2 >= kMinVal) {
      // fp32: the slope is a sum of terms of the size of the initial slope and cannot be resolved much below
      // NW_LS_REL of it; MuJoCo's absolute threshold (reachable in fp64) would only be met by alpha stalling
      const float gtol = fmaxf(gtol_abs, NW_LS_REL * fabsf(p0.d1));
      NwPoint p1 = eval(-p0.d1 / p0.d2);
      if (!(p1.cost <= p0.cost)) p1 = p0;
      if (fabsf(p1.d1) < gtol) {
        alpha = p1.alpha;
      } else {
        // convex restriction: Newton steps in alpha, guarded by the bracket [lo, hi] once it exists
        NwPoint lo = p0, hi = p0;
        bool have_lo = p0.d1 < 0.f, have_hi = !have_lo;
        bool found = false;
        for (int it = 0; it < NW_LS_MAX; it++) {
          if (p1.d1 < 0.f) { if (!have_lo || p1.alpha > lo.alpha) { lo = p1; have_lo = true; } }
          else { if (!have_hi || p1.alpha < hi.alpha) { hi = p1; have_hi = true; } }
          float a = p1.alpha - p1.d1 / p1.d2;
          if (have_lo && have_hi && !(a > lo.alpha && a < hi.alpha)) a = 0.5f * (lo.alpha + hi.alpha);
          // fp32: once the step no longer moves alpha the slope cannot be resolved any further
          if (fabsf(a - p1.alpha) <= 2e-7f * fabsf(p1.alpha)) break;
          p1 = eval(a);
          if (fabsf(p1.d1) < gtol) { found = true; break; }
        }
        if (found) alpha = p1.alpha;
        else if (have_lo && have_hi) alpha = lo.cost < hi.cost ? lo.alpha : hi.alpha;
        else alpha = p1.cost < p0.cost ? p1.alpha : 0.f;
      }
    }
  }
  if (l == 0) { s.scratch[0] = alpha; s.scratch[1] = 0.f; }
  MRE_DBG_STAMP(7, 1);
#if defined(MRE_PHASE_STAMPS) && MRE_PHASE_STAMPS == 7
  if (threadIdx.x == 0) dbg_acc[3] += (unsigned long long)dbg_nev << 4;
#endif
  if (alpha == 0.f) { MRE_SYNC(); return 0.f; }
  qa = fmaf(alpha, sv, qa);
  Ma = fmaf(alpha, Mv, Ma);
  if (l < NVP) { s.qacc[l] = qa; s.nw_Ma[l] = Ma; }
  for (int i = l; i < nefc; i += 64) s.jar[i] = fmaf(alpha, s.jv[i], s.jar[i]);
  MRE_SYNC();
  const float cost = nw_update_gradient<PYR>(s, l, c, nscalar, ncon);
  const float gr = l < NVP ? s.nw_grad[l] : 0.f;
  const float gn = sqrtf(wave_sum(gr * gr));
  if (l == 0) s.scratch[1] = gn;
  MRE_SYNC();
  MRE_DBG_STAMP(7, 2);
  return cost;
}
MRE_PHASE_FN float nw_search_move(ModelP M, Sm& s, int l) { return nw_search_move_impl<false>(M, s, l); }
MRE_PHASE_FN float nw_search_move_pyramidal(ModelP M, Sm& s, int l) { return nw_search_move_impl<true>(M, s, l); }

// ------------------------------------------------------------- mj_fwdConstraint (Newton)
// Runs from the kernel body (the phases above are real functions and never nest calls).
// On exit: s.qacc, s.qfrc_con = J' f, s.solver_iters.
//
// Termination.  mj_solPrimal stops on scale * (cost decrease of the last iteration) < tolerance or
// scale * |grad| < tolerance (1e-8).  Neither can be evaluated in fp32: the cost is a sum of terms up
// to 1e4 (resolution 1e-3), the gradient of the arm dofs carries 1e-5 N m of rounding.  The Newton
// decrement d = grad' H^-1 grad can -- it is formed from the gradient and the search direction with
// no cancellation, and d / 2 IS the decrease the next iteration would achieve: the loop stops on
// scale * d / 2 < tolerance, the same test one iteration ahead.  (Stopping on the fp32 cost
// difference left residual forces of ~3e-5 N m on the finger links, whose inertia is 1e-5 kg m^2:
// a drift of 1e-4 .. 3e-3 rad over 1000 steps against the oracle.)  The check costs one more
// direction, which re-uses the factor when the active set did not change.
#ifdef MRE_PHASE_STAMPS
#define NW_STAMP(k)                                                          \
  do {                                                                       \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();            \
    if ((8 + (k)) / 4 == MRE_PHASE_STAMPS) stamp_acc[(k) % 4] += now_ - stamp_t; \
    stamp_t = now_;                                                          \
  } while (0)
MRE_DEV void newton_solve(ModelP M, Sm& s, int l, unsigned long long* stamp_acc, unsigned long long& stamp_t) {
#else
#define NW_STAMP(k) do {} while (0)
MRE_DEV void newton_solve(ModelP M, Sm& s, int l) {
#endif
  const float tol = M->opt_rec.tolerance;
  const int max_iter = M->opt_rec.iterations;
  const int nscalar = 7 + s.nl, ncon = s.ncon;
  float msum = M->opt_rec.M0_diag_robot_sum;
  for (int p = 0; p < s.nprops; p++)
    msum += 3.f * s.prop_mass[p] + s.prop_inertia[p][0] + s.prop_inertia[p][1] + s.prop_inertia[p][2];
  const float scale = 1.0f / msum;
  const bool pyr = M->opt_rec.cone == 0;
  if (pyr) nw_setup_pyramidal(M, s, l);
  else nw_setup(M, s, l);
  NW_STAMP(0);
  // The decrement test runs at MuJoCo's own tolerance.  (Round 2 ran it a decade lower to shrink the residual force
  // a solve that stops AT the threshold leaves on the finger mechanism; the fp64 polish of the robot block now
  // removes that residual whatever the iteration leaves: NW_TOL_FACTOR 0.1 / 1 / 10 give the same parity figures
  // and 1.81 / 1.78 / 1.75 iterations per step.)
#ifndef NW_TOL_FACTOR
#define NW_TOL_FACTOR 1.0f
#endif
  const float tol_eff = NW_TOL_FACTOR * tol;
  NwMasks mf = {0ull, 0ull, 0ull}, mprev = {~0ull, ~0ull, ~0ull};
  bool have_factor = false, force_full = false;
  float prev_dec = 3.0e38f;
  int iter = 0, nfull = 0, stalls = 0;
  while (iter < max_iter) {
    const NwMasks mk = nw_masks(s, l, nscalar, ncon);
    // (a contact in the middle zone makes H a function of the iterate, not only of the active set: its factor
    // is never re-used -- MuJoCo likewise rebuilds the cone Hessians every iteration)
    const bool reuse = have_factor && !force_full && mk == mf && mk.cc == 0ull;
    if (reuse) {
      nw_direction_reuse(M, s, l);
      NW_STAMP(2);
    } else {
      nw_direction(M, s, l);
      mf = mk; have_factor = true; nfull++;
      NW_STAMP(1);
    }
    const float dec = s.scratch[2];
    if (!(dec == dec)) break;                          // non-finite: keep the last iterate
    if (0.5f * scale * dec < tol_eff) break;           // converged
    if (mk == mprev && dec > 0.1f * prev_dec) {
      // same active set, poor contraction: a stale factor gets a fresh try from the same iterate;
      // with a fresh factor and the decrement already within two decades of the tolerance it is the
      // rounding floor (two strikes), otherwise ordinary slow progress far from the optimum
      if (reuse) { force_full = true; continue; }
      if (0.5f * scale * dec < 100.f * tol_eff && ++stalls >= 2) break;
    }
    prev_dec = dec; mprev = mk; force_full = false;
    if (pyr) nw_search_move_pyramidal(M, s, l);
    else nw_search_move(M, s, l);
    NW_STAMP(3);
    const float alpha = s.scratch[0];
    if (alpha == 0.f) {
      if (reuse) { force_full = true; continue; }
      break;
    }
    iter++;
    // A full Newton step (alpha = 1) with an exact Hessian that lands in the same active set has
    // minimised the very quadratic piece the new point lies in: converged, no check needed.  (Cone
    // contacts make H depend on the iterate; with them the decrement decides.)
    if (!reuse && mk.cc == 0ull && fabsf(alpha - 1.0f) < 1e-4f && nw_masks(s, l, nscalar, ncon) == mk) break;
  }
  if (l < NVP && !(l < NV)) s.qacc[l] = 0.f;
  if (l == 0) s.solver_iters = iter | (nfull << 8);
  MRE_SYNC();
}

// ------------------------------------------------------------- robot polish
// What the float32 Newton iteration cannot deliver is the acceleration of the robot's light or stiffly held parts.
// The finger rows of the gradient are sums of +-0.75 N m (25 N of closure force on 3 cm levers) that leave ~1e-3 N m,
// so the converged iterate carries ~5e-8 N m of rounding there -- on the 2F-85's gram-sized links an error of 1e-4 ..
// 1e-3 rad/s^2 per step (tests/diagnostics/finger_onestep.py), which the follower mode (5 rad/s, damping ratio
// 0.06) integrates to 1e-4 .. 2e-4 rad within 1000 steps; an arm link pressed on the table or a cube (100 N on a
// row with R = 1e-4) leaves 1e-3 .. 7e-3 rad/s^2 on the ARM dofs, which shakes the fingers the arm carries.  The
// cure is one exact Newton step on the robot's fifteen dofs with the cubes' accelerations held: the robot rows of the
// gradient and the 15 x 15 robot block of H = M + J' D J (+ cone Hessians) are formed in fp64 FROM THE SAME float32
// arrays the solver used (Md, Jr, R, aref, qfrc_smooth: their single roundings do not matter -- the oracle with all
// of them rounded to float32 stays within 1.6e-5 of itself over 1000 steps; what matters is that the block is solved
// exactly for them: tests/diagnostics/finger_precision_study.py "e2e-7,1e-3,2"), the block is eliminated in fp64 with
// row i in the registers of lane i (pivot rows by v_readlane), and the robot's accelerations leave as doubles
// (Sm::nw_Mv reused) for the integrator.
// Rows: the 7 equality rows, the joint-limit rows (active set as the solver left it) and every contact with a robot
// part (forces and 3 x 3 weights -- diag(D) in the quadratic zone, the cone Hessian in the middle zone -- re-evaluated
// in fp64 at the iterate).  Returns true when the doubles are valid (false: more than NW_POLISH_CON robot contacts).
MRE_DEV double rdlane_d(double v, int lane) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}
MRE_DEV double rcp_d(double x) {   // 1 / x: v_rcp_f64 and two Newton steps (the IEEE division sequence is 25 instructions)
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}
MRE_PHASE_FN bool nw_robot_polish(ModelP M, Sm& s, int l) {
  static_assert(offsetof(Sm, W) % 8 == 0 && offsetof(Sm, nw_Mv) % 8 == 0, "fp64 views of W / nw_Mv");
  constexpr int MAXROW = 7 + NRV;   // equality + every joint at a limit
  constexpr int NW_POLISH_CON = 32; // robot contacts at most
  static_assert(sizeof(((Sm*)0)->W) >= 8 * (2 * MAXROW + 10 * NW_POLISH_CON), "exchange area");
  static_assert(sizeof(((Sm*)0)->nw_Mv) >= 8 * NRV, "fp64 accelerations out");
  double* const frow = reinterpret_cast<double*>(&s.W[0]);   // [MAXROW] force of scalar row r
  double* const drow = frow + MAXROW;                         // [MAXROW] D of row r if it is active, else 0
  double* const fcon = drow + MAXROW;                         // [NW_POLISH_CON][10]: force 3, weight 6 (00 01 02 11 12 22), robot slot
  double* const a64 = reinterpret_cast<double*>(&s.nw_Mv[0]); // [NRV] out
  const int nscalar = 7 + s.nl, ncon = s.ncon;
  // ---- lane = contact: the ones with a robot part, compacted by a ballot prefix count
  // `full`: a contact touches an ARM body, so the arm block of H carries a stiff row and the arm dofs are polished
  // with the fingers; otherwise the arm's float32 accelerations are good to 2e-7 of their size (harmless: the study's
  // "e2e-7,0,0") and only the eight finger dofs are eliminated -- a quarter of the work
  constexpr int F0 = GRIP_BODY0 - 1;
  int nrc = 0;
  bool full = false;
  {
    const int rs = l < ncon ? (int)s.con_rslot[l] : HDR_NONE;
    const bool mine = rs != HDR_NONE;
    const unsigned long long m = __ballot(mine);
    nrc = __popcll(m);
    if (nrc > NW_POLISH_CON) return false;
    const int cb1 = mine ? (int)s.con_b1[l] : 0, cb2 = mine ? (int)s.con_b2[l] : 0;
    full = __ballot(mine && ((cb1 >= 1 && cb1 < GRIP_BODY0) || (cb2 >= 1 && cb2 < GRIP_BODY0))) != 0ull;
#ifdef MRE_POLISH_FULL
    full = true;   // A/B switch (tools/build_variant.py): every env polishes all 15 robot dofs
#endif
    if (mine) {
      const int k = __popcll(m & ((1ull << l) - 1ull));
      const int i = nscalar + 3 * l, h = s.hdr[i];
      const int pa = (h >> 8) & 0xF, pb = (h >> 12) & 0xF;
      double j[3], D[3];
#pragma unroll
      for (int r = 0; r < 3; r++) {
        double acc = -(double)s.efc_aref[i + r];
#pragma unroll
        for (int c = 0; c < NRV; c++) acc += (double)s.Jr[rs + r][c] * (double)s.qacc[c];
        if (pa < NPROP) { const float* ja = jpA(s, i + r); for (int c = 0; c < 6; c++) acc += (double)ja[c] * (double)s.qacc[NRV + 6 * pa + c]; }
        if (pb < NPROP) { const float* jb = jpB(s, i + r); for (int c = 0; c < 6; c++) acc += (double)jb[c] * (double)s.qacc[NRV + 6 * pb + c]; }
        j[r] = acc;
        D[r] = rcp_d((double)s.efc_R[i + r]);
      }
      // mj_constraintUpdate for one elliptic contact (nw_contact), fp64
      const double fr = (double)s.con_fric[l], mu = fr * sqrt((double)s.efc_R[i + 1] / (double)s.efc_R[i]);
      const double U1 = j[1] * fr, U2 = j[2] * fr, Nn = j[0] * mu, T = sqrt(U1 * U1 + U2 * U2);
      double* o = fcon + 10 * k;
#pragma unroll
      for (int t = 0; t < 9; t++) o[t] = 0.0;
      o[9] = (double)rs;
      if (M->opt_rec.cone == 0) {
        // pyramidal cone: nw_pyramid in fp64
        const double e[4] = {j[0] + fr * j[1], j[0] - fr * j[1], j[0] + fr * j[2], j[0] - fr * j[2]};
        double a[4], n[4];
#pragma unroll
        for (int t = 0; t < 4; t++) { a[t] = e[t] < 0.0 ? e[t] : 0.0; n[t] = e[t] < 0.0 ? 1.0 : 0.0; }
        o[0] = -D[0] * (a[0] + a[1] + a[2] + a[3]);
        o[1] = -D[0] * fr * (a[0] - a[1]);
        o[2] = -D[0] * fr * (a[2] - a[3]);
        o[3] = D[0] * (n[0] + n[1] + n[2] + n[3]);
        o[4] = D[0] * fr * (n[0] - n[1]);
        o[5] = D[0] * fr * (n[2] - n[3]);
        o[6] = D[0] * fr * fr * (n[0] + n[1]);
        o[8] = D[0] * fr * fr * (n[2] + n[3]);
      } else if (Nn >= mu * T || (T <= 0.0 && Nn >= 0.0)) {
        // top zone: no force
      } else if (mu * Nn + T <= 0.0 || (T <= 0.0 && Nn < 0.0)) {
        o[0] = -D[0] * j[0]; o[1] = -D[1] * j[1]; o[2] = -D[2] * j[2];
        o[3] = D[0]; o[6] = D[1]; o[8] = D[2];
      } else {
        const double Dm = D[0] / fmax(mu * mu * (1.0 + mu * mu), 1e-15), NT = Nn - mu * T, iT = 1.0 / T;
        o[0] = -Dm * NT * mu;
        o[1] = -o[0] * iT * U1 * fr;
        o[2] = -o[0] * iT * U2 * fr;
        const double a = mu * Nn * iT * iT * iT, dgn = mu * mu - mu * Nn * iT;
        o[3] = Dm * mu * mu;
        o[4] = Dm * mu * fr * (-mu * U1 * iT);
        o[5] = Dm * mu * fr * (-mu * U2 * iT);
        o[6] = Dm * fr * fr * (a * U1 * U1 + dgn);
        o[7] = Dm * fr * fr * (a * U1 * U2);
        o[8] = Dm * fr * fr * (a * U2 * U2 + dgn);
      }
    }
  }
  // ---- lane = scalar row: J a - aref and the force, fp64
  if (l < nscalar) {
    double jar = -(double)s.efc_aref[l];
#pragma unroll
    for (int j = 0; j < NRV; j++) jar += (double)s.Jr[l][j] * (double)s.qacc[j];
    const bool act = l < 7 || s.rstate[l] == NW_QUAD;
    const double D = act ? rcp_d((double)s.efc_R[l]) : 0.0;
    frow[l] = -D * jar;
    drow[l] = D;
  }
  MRE_SYNC();
  // ---- lane = robot dof: its row of the Hessian block and of the gradient.  Without `full` the block is the finger
  // block: arm lanes carry x = 0, and the arm columns of the finger rows are never read
  const int d = l < NRV ? l : 0;
  const bool row = l < NRV && (full || l >= F0);
  double hrow[NRV], g = 0.0;
#pragma unroll
  for (int j = 0; j < NRV; j++) hrow[j] = row ? (double)s.Md[d][j] : 0.0;
  if (row) {
    g = -(double)s.qfrc_smooth[d];
#pragma unroll
    for (int j = 0; j < NRV; j++) g += (double)s.Md[d][j] * (double)s.qacc[j];
    for (int r = 0; r < nscalar; r++) {
      const double jd = (double)s.Jr[r][d];
      g -= jd * frow[r];
      const double t = drow[r] * jd;
      if (full) {
#pragma unroll
        for (int j = 0; j < F0; j++) hrow[j] += t * (double)s.Jr[r][j];
      }
#pragma unroll
      for (int j = F0; j < NRV; j++) hrow[j] += t * (double)s.Jr[r][j];
    }
    for (int k = 0; k < nrc; k++) {
      const double* o = fcon + 10 * k;
      const int rs = (int)o[9];
      const double j0 = (double)s.Jr[rs][d], j1 = (double)s.Jr[rs + 1][d], j2 = (double)s.Jr[rs + 2][d];
      g -= j0 * o[0] + j1 * o[1] + j2 * o[2];
      const double t0 = j0 * o[3] + j1 * o[4] + j2 * o[5], t1 = j0 * o[4] + j1 * o[6] + j2 * o[7],
                   t2 = j0 * o[5] + j1 * o[7] + j2 * o[8];
      if (full) {
#pragma unroll
        for (int j = 0; j < F0; j++)
          hrow[j] += t0 * (double)s.Jr[rs][j] + t1 * (double)s.Jr[rs + 1][j] + t2 * (double)s.Jr[rs + 2][j];
      }
#pragma unroll
      for (int j = F0; j < NRV; j++)
        hrow[j] += t0 * (double)s.Jr[rs][j] + t1 * (double)s.Jr[rs + 1][j] + t2 * (double)s.Jr[rs + 2][j];
    }
  }
  // ---- elimination: row i in lane i, pivot row k read from lane k; x = -H^-1 g
  double x = -g;
  double pinv[NRV];   // reciprocal pivots (wave-uniform), kept for the back substitution
#pragma unroll
  for (int k = 0; k < NRV; k++) pinv[k] = 1.0;
  if (full) {
#pragma unroll
    for (int k = 0; k < F0; k++) {
      pinv[k] = rcp_d(rdlane_d(hrow[k], k));
      const double xk = rdlane_d(x, k);
      const double mlt = (l > k && l < NRV) ? hrow[k] * pinv[k] : 0.0;
#pragma unroll
      for (int j = k + 1; j < NRV; j++) hrow[j] -= mlt * rdlane_d(hrow[j], k);
      x -= mlt * xk;
    }
  }
#pragma unroll
  for (int k = F0; k < NRV; k++) {
    pinv[k] = rcp_d(rdlane_d(hrow[k], k));
    if (k == NRV - 1) break;
    const double xk = rdlane_d(x, k);
    const double mlt = (l > k && l < NRV) ? hrow[k] * pinv[k] : 0.0;
#pragma unroll
    for (int j = k + 1; j < NRV; j++) hrow[j] -= mlt * rdlane_d(hrow[j], k);
    x -= mlt * xk;
  }
#pragma unroll
  for (int k = NRV - 1; k >= F0; k--) {
    const double xk = rdlane_d(x, k) * pinv[k];   // (uniform: every lane forms the same product)
    if (l == k) x = xk;
    else if (l < k && row) x -= hrow[k] * xk;
  }
  if (full) {
#pragma unroll
    for (int k = F0 - 1; k >= 0; k--) {
      const double xk = rdlane_d(x, k) * pinv[k];
      if (l == k) x = xk;
      else if (l < k) x -= hrow[k] * xk;
    }
  }
  if (l < NRV) {
    const double a = (double)s.qacc[l] + x;    // (x = 0 on the arm lanes of a finger-only polish)
    a64[l] = a;
    s.qacc[l] = (float)a;
  }
  MRE_SYNC();
  return true;
}

}  // namespace mre
