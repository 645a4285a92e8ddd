// mre_solver.h -- collision driver, constraint assembly and the PGS solve for one
// environment per wavefront.  Included by mre_kernels.hip after `struct Sm`.
//
// Constraint rows (MuJoCo order): 7 equality rows (2 connect x 3 + 1 joint),
// active joint limits, then 3 rows (normal + 2 tangents, elliptic cone) per
// active contact.  Row storage exploits the scene's block structure: a row
// touches at most the 15 robot dofs ("robot part", Jr/Br pools, only for rows
// that involve a robot body) and at most two cubes ("prop parts", 6 dofs each).
// The cube blocks of the mass matrix are diagonal in MuJoCo's c-frame
// (diag(m,m,m,Ixx,Iyy,Izz)), so M^-1 J' needs storage for the robot part only.
//
// PGS is run matrix-free: lanes own dofs and carry a = M^-1 J' f and w = J' f in
// registers.  Rows are grouped in blocks (a contact's three rows, or three consecutive
// scalar rows) and the blocks of a sweep are scheduled over "islands" (the robot's 16
// lanes, 8 lanes per cube): blocks touching disjoint islands run in the same step, blocks
// sharing an island keep MuJoCo's order, so the iterates are identical (in exact
// arithmetic) to MuJoCo's sequential PGS on the explicit A = J M^-1 J' + R that the CPU
// oracle builds.  A step is three island dot products (DPP), the block update, and a
// rank-3 update of a and w.
#pragma once

namespace mre {

constexpr int HDR_NONE = 0xFF;
constexpr int BLK_NONE = 0x7F;
constexpr int SCHED_NONE = 0xFF;
// solver operand table (solve_constraints): entries for MAXBLK steps x 5 islands, one all-off
// entry, then a pad of zeros that idle islands read their Jacobian rows from (TAB_BYTES in all)
constexpr int TAB_OFF = MAXBLK * 5;
constexpr int TAB_ZEROS = 48;
static_assert(TAB_BYTES == 8 * (TAB_OFF + 1) + 4 * TAB_ZEROS, "operand table size");

#ifndef MRE_NEWTON
MRE_DEV void build_schedule(ModelP M, Sm& s);
#endif
// bit of the unordered cube pair {p, q} in Sm::cpl_cubes: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
MRE_DEV constexpr int cube_pair_bit(int p, int q) {
  const int a = p < q ? p : q, b = p < q ? q : p;
  return a == 0 ? b - 1 : (a == 1 ? b + 1 : 5);
}

MRE_DEV float prop_invM(const Sm& s, int p, int k) {
  return 1.0f / ((k < 3) ? s.prop_mass[p] : s.prop_inertia[p][k - 3]);
}

MRE_DEV void geom_pose(ModelP M, const Sm& s, int g, float* p, float* R, float* size,
                       float* rbound) {
  const int b = M->geom_body[g];
  float tmp[3], q[4];
  m3mulv(tmp, s.xmat[b], M->geom_pos[g]);
  v3add(p, s.xpos[b], tmp);
  qmul(q, s.xquat[b], M->geom_quat[g]);
  q2mat(R, q);
  const int pid = M->geom_propid[g];
  if (pid >= 0) {
    v3copy(size, s.prop_size[pid]);
    *rbound = v3norm(size);
  } else {
    v3copy(size, M->geom_size[g]);
    *rbound = M->geom_rbound[g];
  }
}

// ------------------------------------------------------------------ mj_collision
// lane = entry of the static pair table, one wave-wide pass per 64 pairs; keeps ACTIVE contacts
// only (dist < margin - gap), in pair order, capped at NCON_MAX.
// detect: keep every DETECTED contact (dist < margin: what physics.data.contact lists,
// environment/prop_initializer.py:121-140) instead of the active ones (dist < margin - gap)
// centre and bounding radius of geom g (the part of geom_pose the broad phase needs)
MRE_DEV void geom_center(ModelP M, const Sm& s, int g, float* p, float* rbound) {
  const int b = M->geom_body[g];
  float tmp[3];
  m3mulv(tmp, s.xmat[b], M->geom_pos[g]);
  v3add(p, s.xpos[b], tmp);
  const int pid = M->geom_propid[g];
  *rbound = pid >= 0 ? v3norm(s.prop_size[pid]) : M->geom_rbound[g];
}

// Two stages.  Broad phase: lane = entry of the static pair table (one wave-wide pass per 64 pairs), bounding
// sphere / plane distance test on the geom centres only, survivors compacted IN TABLE ORDER into a byte list.
// Narrow phase: lane = survivor (one pass for up to 64 of them; a scene has a dozen), full geom frames,
// box-box / plane-box, then the per-lane candidate counts are turned into output slots by a ballot prefix
// sum, so contacts come out in pair order exactly as a pair-by-pair loop would list them.
// A lane whose box_box returns its candidates in registers (FACE_IN_REGS, mre_collide.h: an unclipped face contact)
// filters, reduces and stores them from there, in the order and with the expressions of the LDS loops;
// clip_always (F_CLIP_ALWAYS, wave-uniform) sends every lane through the LDS path.
// The two stages are phase functions of their own and the loop over the narrow passes (one, as a rule) is the
// caller's: inside one function the compiler hoists every address and constant of the narrow phase out of that loop
// and carries the register candidates round it -- 246 VGPRs in one function, 72 and 166 in two (profiles/NOTES.md, round 11).
// Broad phase: returns the number of survivors listed in s.iscr.
MRE_PHASE_FN int collide_broad(ModelP M, Sm& s, int l, bool detect) {
  // per-lane clip buffers alias the Jacobian pools (contiguous Jp|Jr|Br, unused until assembly)
  // [JpA .. sched] is one contiguous block of arrays that are only written after collision
  static_assert(offsetof(Sm, hdr) + sizeof(((Sm*)0)->hdr) - offsetof(Sm, JpA) >= sizeof(float) * 64 * COLL_BUF,
                "clip buffers do not fit");
  static_assert(NPAIR <= 256 && sizeof(((Sm*)0)->iscr) >= NPAIR, "survivor list: one byte per pair");
  MRE_DBG_T0();
  uint8_t* list = reinterpret_cast<uint8_t*>(s.iscr);
  const unsigned long long lt = (1ull << l) - 1ull;   // lanes below this one
  int nsurv = 0;
  for (int pass = 0; pass < NPAIR / 64; pass++) {
    const int pr = l + 64 * pass;
    // the pair's record: independent loads, one trip to memory (PairRec, mre_dev.h)
    const auto* R = &M->pair_rec[pr];
    const int g1 = R->g1, b1 = R->b1, b2 = R->b2, pid1 = R->pid1, pid2 = R->pid2, type1 = R->type1;
    const float lp1[3] = {R->pos1[0], R->pos1[1], R->pos1[2]}, lp2[3] = {R->pos2[0], R->pos2[1], R->pos2[2]};
    const float mrb1 = R->rb1, mrb2 = R->rb2, margin = R->margin, gap = R->gap;
    const float lq1[4] = {R->quat1[0], R->quat1[1], R->quat1[2], R->quat1[3]};
    bool live = false;
    if (g1 >= 0 && (pid1 < 0 || pid1 < s.nprops) && (pid2 < 0 || pid2 < s.nprops)) {
      const float inc = detect ? margin : margin - gap;
      float p1[3], p2[3], df[3], tmp[3];
      m3mulv(tmp, s.xmat[b1], lp1); v3add(p1, s.xpos[b1], tmp);
      m3mulv(tmp, s.xmat[b2], lp2); v3add(p2, s.xpos[b2], tmp);
      const float rb1 = pid1 >= 0 ? v3norm(s.prop_size[pid1]) : mrb1, rb2 = pid2 >= 0 ? v3norm(s.prop_size[pid2]) : mrb2;
      v3sub(df, p2, p1);
      if (type1 == 0) {
        float q[4], R1[9];
        qmul(q, s.xquat[b1], lq1);
        q2mat(R1, q);
        const float nn[3] = {R1[2], R1[5], R1[8]};
        live = v3dot(df, nn) - rb2 <= inc;
      } else {
        const float r = rb1 + rb2 + inc;
        live = v3dot(df, df) <= r * r;
      }
    }
    const unsigned long long m = __ballot(live);
    if (live) list[nsurv + __popcll(m & lt)] = (uint8_t)pr;
    nsurv += __popcll(m);
  }
  if (l == 0) s.ncon = 0;
  MRE_SYNC();
  MRE_DBG_STAMP(6, 0);
  return nsurv;
}
// One narrow pass over the survivors c0 .. c0 + 63; base: contacts kept by the earlier passes.  Returns the contacts
// found so far (more than NCON_MAX: overflow, nothing further is stored).
MRE_PHASE_FN int collide_narrow(ModelP M, Sm& s, int l, bool detect, bool clip_always, int c0, int nsurv, int base) {
  MRE_DBG_T0();
  float* buf = &s.JpA[0][0] + l * COLL_BUF;
  const uint8_t* list = reinterpret_cast<const uint8_t*>(s.iscr);
  const unsigned long long lt = (1ull << l) - 1ull;   // lanes below this one
  {
    const int pr = (c0 + l < nsurv) ? list[c0 + l] : -1;
    float normal[3] = {0.f, 0.f, 1.f};
    int n = 0;
    FaceCand rc;         // read only under the mask bits of rm
    unsigned rm = 0u;
    if (pr >= 0) {
      const auto* R = &M->pair_rec[pr];
      const int b1 = R->b1, b2 = R->b2, pid1 = R->pid1, pid2 = R->pid2, type1 = R->type1;
      const float lp1[3] = {R->pos1[0], R->pos1[1], R->pos1[2]}, lp2[3] = {R->pos2[0], R->pos2[1], R->pos2[2]};
      const float lq1[4] = {R->quat1[0], R->quat1[1], R->quat1[2], R->quat1[3]};
      const float lq2[4] = {R->quat2[0], R->quat2[1], R->quat2[2], R->quat2[3]};
      const float ms1[3] = {R->size1[0], R->size1[1], R->size1[2]}, ms2[3] = {R->size2[0], R->size2[1], R->size2[2]};
      const float margin = R->margin, gap = R->gap;
      float p1[3], R1[9], s1[3], p2[3], R2[9], s2[3], tmp[3], q[4];
      m3mulv(tmp, s.xmat[b1], lp1); v3add(p1, s.xpos[b1], tmp);
      qmul(q, s.xquat[b1], lq1); q2mat(R1, q);
      m3mulv(tmp, s.xmat[b2], lp2); v3add(p2, s.xpos[b2], tmp);
      qmul(q, s.xquat[b2], lq2); q2mat(R2, q);
      if (pid1 >= 0) v3copy(s1, s.prop_size[pid1]); else v3copy(s1, ms1);
      if (pid2 >= 0) v3copy(s2, s.prop_size[pid2]); else v3copy(s2, ms2);
      const float inc = detect ? margin : margin - gap;
      MRE_DBG_STAMP(6, 1);
      if ((R->single >> 8) == 2) n = cyl_box(p1, R1, s1, p2, R2, s2[0], s2[2], inc, normal, buf);   // geom 2 is a cylinder
      else if (type1 == 0) n = plane_box(p1, R1, p2, R2, s2, inc, normal, buf);
      else n = box_box(p1, R1, s1, p2, R2, s2, inc, normal, buf, clip_always, rc, rm);
      MRE_DBG_STAMP(6, 2);
      // instantiate only contacts with dist < includemargin
      int m = 0;
      if (rm & FACE_IN_REGS) {
#pragma unroll
        for (int v = 0; v < 4; v++) {
          if (((rm >> v) & 1u) != 0u && rc.d[v] < inc) m++;
          else rm &= ~(1u << v);
        }
      } else {
        for (int c = 0; c < n; c++)
          if (cand_dist(buf, c) < inc) {
            if (m != c) {
              for (int k = 0; k < 3; k++) cand_xyz(buf, m)[k] = cand_xyz(buf, c)[k];
              cand_dist(buf, m) = cand_dist(buf, c);
            }
            m++;
          }
      }
      n = m;
    }
#if defined(MRE_PHASE_STAMPS) && MRE_PHASE_STAMPS == 8
    {   // face contacts of the wave, those that stayed in registers, and the same two for pairs with the table (geom 1)
      const bool tbl = pr >= 0 && (M->pair_rec[pr].g1 == 1);
      const unsigned long long fb = __ballot((rm & FACE_BRANCH) != 0u), fr = __ballot((rm & FACE_IN_REGS) != 0u), tb = __ballot(tbl);
      if (l == 0) {
        dbg_acc[0] += (unsigned long long)__popcll(fb) << 4; dbg_acc[1] += (unsigned long long)__popcll(fr) << 4;
        dbg_acc[2] += (unsigned long long)__popcll(fb & tb) << 4; dbg_acc[3] += (unsigned long long)__popcll(fr & tb) << 4;
      }
    }
#endif
    // mesh stand-in pairs keep ONE contact, like MuJoCo's convex-mesh test (formed at the write-out below)
    const bool single = pr >= 0 && n > 1 && (M->pair_rec[pr].single & 0xFF) != 0;
    const int ncand = n;
    if (single) n = 1;
    // exclusive prefix sum of n (<= 8) over the lanes, bit by bit through ballots
    int off = base, tot = base;
    for (int bit = 0; bit < 4; bit++) {
      const unsigned long long m = __ballot((n >> bit) & 1);
      off += __popcll(m & lt) << bit;
      tot += __popcll(m) << bit;
    }
    if (l == 0) {
      s.ncon = tot < NCON_MAX ? tot : NCON_MAX;
      if (tot > NCON_MAX) s.overflow = 1;
    }
    if (single) {
      // depth of the deepest candidate, position = the centroid of the active candidates weighted by their depth
      // below the threshold (the deepest point alone jumps between the corners of the clip polygon when two faces are
      // nearly parallel; oracle: collision()).  Written into candidate slot 0, which the loop below stores.
      const float incw = M->pair_rec[pr].margin - M->pair_rec[pr].gap;
      if (rm & FACE_IN_REGS) {
        float wsum = 0.f, px = 0.f, py = 0.f, pz = 0.f, dmin = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
        bool first = true;
#pragma unroll
        for (int v = 0; v < 4; v++)
          if (((rm >> v) & 1u) != 0u) {
            const float dc = rc.d[v];
            if (first || dc < dmin) { dmin = dc; bx = rc.x[v]; by = rc.y[v]; bz = rc.z[v]; }
            first = false;
            const float w = incw - dc;
            if (w > 0.f) { wsum += w; px += w * rc.x[v]; py += w * rc.y[v]; pz += w * rc.z[v]; }
          }
        if (wsum > 0.f) { const float iw = 1.0f / wsum; px *= iw; py *= iw; pz *= iw; }
        else { px = bx; py = by; pz = bz; }
        rc.x[0] = px; rc.y[0] = py; rc.z[0] = pz; rc.d[0] = dmin;
        rm = FACE_IN_REGS | 1u;
      } else {
        float wsum = 0.f, px = 0.f, py = 0.f, pz = 0.f, dmin = cand_dist(buf, 0);
        int best = 0;
        for (int c = 0; c < ncand; c++) {
          const float dc = cand_dist(buf, c);
          if (dc < dmin) { dmin = dc; best = c; }
          const float w = incw - dc;
          if (w > 0.f) { wsum += w; px += w * cand_xyz(buf, c)[0]; py += w * cand_xyz(buf, c)[1]; pz += w * cand_xyz(buf, c)[2]; }
        }
        if (wsum > 0.f) { const float iw = 1.0f / wsum; px *= iw; py *= iw; pz *= iw; }
        else { px = cand_xyz(buf, best)[0]; py = cand_xyz(buf, best)[1]; pz = cand_xyz(buf, best)[2]; }
        cand_xyz(buf, 0)[0] = px; cand_xyz(buf, 0)[1] = py; cand_xyz(buf, 0)[2] = pz;
        cand_dist(buf, 0) = dmin;
      }
    }
    if (n > 0) {
      float f[9];
      v3copy(f, normal);
      make_frame(f);
      if (rm & FACE_IN_REGS) {
        int id = off;   // slots in vertex order; past NCON_MAX nothing more is stored
#pragma unroll
        for (int v = 0; v < 4; v++)
          if (((rm >> v) & 1u) != 0u && id < NCON_MAX) {
            s.con_pos[id][0] = rc.x[v]; s.con_pos[id][1] = rc.y[v]; s.con_pos[id][2] = rc.z[v];
            for (int k = 0; k < 9; k++) s.con_frame[id][k] = f[k];
            s.con_dist[id] = rc.d[v];
            s.con_pair[id] = (uint8_t)pr;
            id++;
          }
      } else {
        for (int c = 0; c < n; c++) {
          const int id = off + c;
          if (id >= NCON_MAX) break;
          const float cx0 = cand_xyz(buf, c)[0], cx1 = cand_xyz(buf, c)[1], cx2 = cand_xyz(buf, c)[2];
          s.con_pos[id][0] = cx0; s.con_pos[id][1] = cx1; s.con_pos[id][2] = cx2;
          for (int k = 0; k < 9; k++) s.con_frame[id][k] = f[k];
          s.con_dist[id] = cand_dist(buf, c);
          s.con_pair[id] = (uint8_t)pr;
        }
      }
    }
    MRE_SYNC();
    MRE_DBG_STAMP(6, 3);
    return tot;
  }
}
MRE_DEV void collide(ModelP M, Sm& s, int l, bool detect, bool clip_always) {
  const int nsurv = collide_broad(M, s, l, detect);
  int base = 0;
  for (int c0 = 0; c0 < nsurv; c0 += 64) {
    base = collide_narrow(M, s, l, detect, clip_always, c0, nsurv, base);
    if (base > NCON_MAX) break;   // (overflow: the env is re-run on the large kernel, or reported)
  }
}

// getimpedance (MuJoCo engine_core_constraint.c)
MRE_DEV float impedance(const float* solimp, float pos, float margin) {
  const float dmin = clampf(solimp[0], 0.0001f, 0.9999f), dmax = clampf(solimp[1], 0.0001f, 0.9999f);
  const float width = fmaxf(solimp[2], kMinVal), mid = clampf(solimp[3], 0.0001f, 0.9999f);
  const float power = fmaxf(solimp[4], 1.0f);
  if (dmin == dmax) return 0.5f * (dmin + dmax);
  const float x = fabsf((pos - margin) / width);
  if (x >= 1.0f) return dmax;
  if (x <= 0.0f) return dmin;
  float y;
  if (power == 1.0f) y = x;
  else if (power == 2.0f) {
    // MuJoCo's default solimp power (every row of this scene): a^2 / b^1 without four calls of the general
    // powf (log + exp, a hundred instructions each, which a lane = row loop pays on both sides of x <= mid)
    y = (x <= mid) ? x * x / mid : 1.0f - (1.0f - x) * (1.0f - x) / (1.0f - mid);
  }
  else if (x <= mid) y = powf(x, power) / powf(mid, power - 1.0f);
  else y = 1.0f - powf(1.0f - x, power) / powf(1.0f - mid, power - 1.0f);
  return dmin + y * (dmax - dmin);
}

// accumulate sg * ax . (d point / d q) of a point on robot body b into Jr[rs]
MRE_DEV void jac_robot(ModelP M, Sm& s, int rs, int b, const float* p, const float* ax, float sg) {
  float off[3];
  v3sub(off, p, s.com_robot);
  const int n = M->chain_len[b];
  for (int k = 0; k < n; k++) {
    const int j = M->chain_dof[b][k];
    const float* c = s.cdof[j];
    float t[3];
    v3cross(t, c, off);
    s.Jr[rs][j] += sg * (ax[0] * (c[3] + t[0]) + ax[1] * (c[4] + t[1]) + ax[2] * (c[5] + t[2]));
  }
}
// block record of row i (see Sm::blkrec): record index and row-in-block
MRE_DEV int row_blk(const Sm& s, int i, int& r) {
  const int ns = 7 + s.nl;
  if (i < ns) { r = i % 3; return i / 3; }
  const int cr = i - ns;
  r = cr % 3;
  return 8 + cr / 3;
}
#ifdef MRE_NEWTON
MRE_DEV float& rowR(Sm& s, int i) { return s.efc_R[i]; }
MRE_DEV float& rowB(Sm& s, int i) { return s.efc_aref[i]; }
#else
MRE_DEV float& rowR(Sm& s, int i) { int r; const int b = row_blk(s, i, r); return s.blkrec[b][r]; }
MRE_DEV float& rowB(Sm& s, int i) { int r; const int b = row_blk(s, i, r); return s.blkrec[b][3 + r]; }
MRE_DEV float& rowAinv(Sm& s, int i) { int r; const int b = row_blk(s, i, r); return s.blkrec[b][6 + r]; }
#endif

// prop parts of contact row i: part A (first cube of the contact) is indexed by contact row,
// part B exists only for cube-cube contacts (slot con_bslot)
MRE_DEV float* jpA(Sm& s, int i) { return s.JpA[i - 7 - s.nl]; }
MRE_DEV const float* jpA(const Sm& s, int i) { return s.JpA[i - 7 - s.nl]; }
MRE_DEV float* jpB(Sm& s, int i) { const int cr = i - 7 - s.nl; return s.JpB[3 * s.con_bslot[cr / 3] + cr % 3]; }
MRE_DEV const float* jpB(const Sm& s, int i) { const int cr = i - 7 - s.nl; return s.JpB[3 * s.con_bslot[cr / 3] + cr % 3]; }
// same for a cube body into the prop part `slot` of row i
MRE_DEV void jac_prop(Sm& s, int i, int slot, int b, const float* p, const float* ax, float sg) {
  float off[3];
  v3sub(off, p, s.xpos[b]);
  float* J = slot == 0 ? jpA(s, i) : jpB(s, i);
  for (int k = 0; k < 3; k++) {
    J[k] = sg * ax[k];
    float axk[3] = {s.xmat[b][k], s.xmat[b][3 + k], s.xmat[b][6 + k]}, t[3];
    v3cross(t, axk, off);
    J[3 + k] = sg * v3dot(ax, t);
  }
}

// J_i . vec for an nv-vector in LDS (lane = row helper)
MRE_DEV float row_dot(const Sm& s, int i, const float* vec) {
  const int h = s.hdr[i];
  const int rs = h & 0xFF, pa = (h >> 8) & 0xF, pb = (h >> 12) & 0xF;
  float acc = 0.f;
  if (rs != HDR_NONE)
    for (int j = 0; j < NRV; j++) acc += s.Jr[rs][j] * vec[j];
  if (pa < NPROP)
    { const float* ja = jpA(s, i); for (int k = 0; k < 6; k++) acc += ja[k] * vec[NRV + 6 * pa + k]; }
  if (pb < NPROP)
    { const float* jb = jpB(s, i); for (int k = 0; k < 6; k++) acc += jb[k] * vec[NRV + 6 * pb + k]; }
  return acc;
}

// the same for two vectors at once: the row's Jacobian words are read once (same additions in the same order as two
// row_dot calls: same bits)
MRE_DEV void row_dot2(const Sm& s, int i, const float* v1, const float* v2, float& r1, float& r2) {
  const int h = s.hdr[i];
  const int rs = h & 0xFF, pa = (h >> 8) & 0xF, pb = (h >> 12) & 0xF;
  float a1 = 0.f, a2 = 0.f;
  if (rs != HDR_NONE)
    for (int j = 0; j < NRV; j++) { const float jv = s.Jr[rs][j]; a1 += jv * v1[j]; a2 += jv * v2[j]; }
  if (pa < NPROP) {
    const float* ja = jpA(s, i);
    for (int k = 0; k < 6; k++) { const float jv = ja[k]; a1 += jv * v1[NRV + 6 * pa + k]; a2 += jv * v2[NRV + 6 * pa + k]; }
  }
  if (pb < NPROP) {
    const float* jb = jpB(s, i);
    for (int k = 0; k < 6; k++) { const float jv = jb[k]; a1 += jv * v1[NRV + 6 * pb + k]; a2 += jv * v2[NRV + 6 * pb + k]; }
  }
  r1 = a1; r2 = a2;
}

#ifndef MRE_NEWTON
// Br = M^-1 Jr' (lane = robot slot; register-resident sparse solve unrolled over the dof tree).
// A function of its own: the unrolled solve wants ~100 registers for the factor entries.
MRE_PHASE_FN void solve_robot_rows(Sm& s, int l) {
  for (int rs = l; rs < s.nrrow; rs += 64) {
    float x[NRV];
#pragma unroll
    for (int k = 0; k < NRV; k++) x[k] = s.Jr[rs][k];
    solve_robot_regs(s.qLD, s.qLDinv, x);
#pragma unroll
    for (int k = 0; k < NRV; k++) s.Br[rs][k] = x[k];
  }
  MRE_SYNC();
}

#endif  // !MRE_NEWTON

// ---- connect residual of the gripper linkage in double precision
// The two `connect` rows close each finger's four-bar (follower <-> coupler).  Their residual is a
// 1e-5 m difference of two anchor positions; evaluated from the fp32 world poses (|x| ~ 0.8 m) it
// carries ~5e-8 m of rounding noise, which the stiff reference acceleration (K ~ 2.5e5 1/s^2)
// turns into torques on links of a few grams: measured finger-joint divergence from the fp64 oracle
// 1e-4 .. 3e-2 rad over 1000 steps, although neither the state nor the solver is at fault (the same
// noise injected into the fp64 oracle reproduces it; 1e-9 m does not).  Both anchors hang off the
// same arm link, so the residual is evaluated in THAT link's frame from the four joint angles alone,
// in fp64 (sin / cos by Taylor polynomials, |half angle| < 1), and only then rotated to the world.
constexpr int GRIP0 = GRIP_BODY0;
// (the fp64 evaluation of the two `connect` rows lives next to gripper_local in mre_kernels.hip)

// ------------------------- mj_makeConstraint + mj_makeImpedance + reference + project
MRE_PHASE_FN void assemble_constraints(ModelP M, Sm& s, int l) {
  // ---- joint limits: lane = robot body; at most one side can be violated
  int lim = 0, lim_side = 0;
  const auto* BR = &M->body_rec[l < NRB ? l : 0];   // (the joint's range and flag: one group of loads)
  const int jnt_limited = BR->jnt_limited;
  const float jnt_range[2] = {BR->jnt_range[0], BR->jnt_range[1]};
  if (l >= 1 && l < NRB && jnt_limited) {
    const double q = robot_q(s, l - 1);   // (the full double-float angle, mre_kernels.hip: robot_q)
    if (q - (double)jnt_range[0] < 0.0) { lim = 1; lim_side = -1; }
    else if ((double)jnt_range[1] - q < 0.0) { lim = 1; lim_side = 1; }
  }
  keep_live(jnt_range[0]); keep_live(jnt_range[1]);
  // (rows in joint order: the row index of a violated limit is the number of violated limits on the lanes below)
  const unsigned long long limm = __ballot(lim != 0);
  const int lim_idx = __popcll(limm & ((1ull << l) - 1ull));
  if (l == 0) s.nl = __popcll(limm);
  if (lim) s.lim_info[lim_idx] = l | ((lim_side > 0 ? 1 : 0) << 8);
  // bodies of every contact's geoms (lane = contact): the serial loops below then read LDS only
  // instead of chasing pair -> geom -> body through the model tables once per contact
  if (l < s.ncon) {
    const int pr = s.con_pair[l];
    s.con_b1[l] = (uint8_t)M->pair_rec[pr].b1;
    s.con_b2[l] = (uint8_t)M->pair_rec[pr].b2;
  }
  MRE_SYNC();
#ifndef MRE_NEWTON
  {
    static_assert(sizeof(s.sched) % 4 == 0, "schedule cleared by words");
    unsigned* w = reinterpret_cast<unsigned*>(&s.sched[0][0]);
    for (int e = l; e < (int)(sizeof(s.sched) / 4); e += 64) w[e] = 0x01010101u * (unsigned)SCHED_NONE;
  }
#endif
  // ---- robot-slot assignment and capacity (lane = contact; slots are prefix counts over the contacts below,
  // the list is cut at the first contact that does not fit, exactly as a contact-by-contact loop would)
  {
    const int base = 7 + s.nl, ncon0 = s.ncon;
    const bool on = l < ncon0;
    const int cb1 = on ? s.con_b1[l] : 0, cb2 = on ? s.con_b2[l] : 0;
    const bool rob_any = on && ((cb1 < NRB && cb1 > 0) || (cb2 < NRB && cb2 > 0));
    const bool fing = on && ((cb1 >= GRIP_BODY0 && cb1 < NRB) || (cb2 >= GRIP_BODY0 && cb2 < NRB));
    const unsigned long long fingm = __ballot(fing);
    const bool two_props = on && cb1 >= NRB && cb2 >= NRB;
    const unsigned long long lt = (1ull << l) - 1ull;
    const unsigned long long rmask = __ballot(rob_any), tmask = __ballot(two_props);
    const int my_r = base + 3 * __popcll(rmask & lt), my_b = __popcll(tmask & lt);
    const bool fail = on && (base + 3 * (l + 1) > NEFC_MAX || (rob_any && my_r + 3 > NRROW_MAX) ||
                             (two_props && my_b >= NPP_MAX));
    const unsigned long long fmask = __ballot(fail);
    const int kept = fmask != 0ull ? (int)__builtin_ctzll(fmask) : ncon0;
    if (l < kept) {
      s.con_rslot[l] = rob_any ? my_r : HDR_NONE;
      s.con_bslot[l] = two_props ? my_b : 0;
    }
    MRE_SYNC();
    if (l == 0) {
      const unsigned long long below = kept >= 64 ? ~0ull : ((1ull << kept) - 1ull);
      if (fmask != 0ull) s.overflow = 1;
      s.ncon = kept;
      s.nefc = base + 3 * kept;
      s.nrrow = base + 3 * __popcll(rmask & below);
      s.npp = __popcll(tmask & below);
      s.finger_contact = (fingm & below) != 0ull;
#ifdef MRE_NEWTON
      s.nsched = 0; s.nblk = 0;  // (contact lists of the Newton solver: nw_build_lists, mre_newton.h)
#else
      build_schedule(M, s);
#endif
    }
  }
  MRE_SYNC();
  const int nefc = s.nefc, nl = s.nl;
  // ---- zero robot slots and the scalar-triple records (rows past a short last triple stay 0)
  for (int e = l; e < s.nrrow * NRV; e += 64) (&s.Jr[0][0])[e] = 0.f;
#ifndef MRE_NEWTON
  for (int e = l; e < 8 * 16; e += 64) (&s.blkrec[0][0])[e] = 0.f;
#endif
  MRE_SYNC();
  // ---- rows (lane = row)
  for (int i = l; i < nefc; i += 64) {
    int rs = HDR_NONE, pa = 0xF, pb = 0xF;
    float pos = 0.f, margin = 0.f, diag = 0.f, imp_pos = 0.f;
    bool fric_row = false;
    float R0scale = 1.0f;
    // ---- the row's parameters (RowRec, mre_dev.h: solref, solimp, margin, gap, friction, diagonal weights), the range
    // of a limit row's joint and the options the row reads, fetched HERE in one group of loads: their latency runs
    // under the Jacobian work below instead of being paid, table by table, where each value is used
    const int eqi = i < 6 ? i / 3 : 2;     // (rows 0..6: equality constraint of the row)
    const int limb = (i >= 7 && i < 7 + nl) ? (s.lim_info[i - 7] & 0xFF) : 0;   // (limit rows: the joint's body)
    const int rrec = i < 7 ? eqi : (i < 7 + nl ? ROWREC_JNT + limb : ROWREC_PAIR + s.con_pair[(i - 7 - nl) / 3]);
    const auto* RR = &M->row_rec[rrec];
    const float solref[2] = {RR->solref[0], RR->solref[1]};
    const float solimp[5] = {RR->solimp[0], RR->solimp[1], RR->solimp[2], RR->solimp[3], RR->solimp[4]};
    const float rec_margin = RR->margin, rec_gap = RR->gap, rec_friction = RR->friction, invw1 = RR->invw1, invw2 = RR->invw2;
    const float lim_range[2] = {M->body_rec[limb].jnt_range[0], M->body_rec[limb].jnt_range[1]};
    const float opt_timestep = M->opt_rec.timestep, opt_impratio = M->opt_rec.impratio;
    const int opt_cone = M->opt_rec.cone;
    if (i < 7) {
      rs = i;
      const int e = eqi;
      // the constraint's record (EqRec), whole, before the row's two kinds part ways
      const auto* E = &M->eq_rec[e];
      const int b1 = E->b1, b2 = E->b2;
      const int root = E->root, pb1 = E->pb1, pb2 = E->pb2;   // (root: the arm link the linkage hangs off)
      const float pc[5] = {E->data[0], E->data[1], E->data[2], E->data[3], E->data[4]};
      const float q0_1 = E->qpos0_1, q0_2 = E->qpos0_2;
      // (the dofs from the base to the root link, in the order of chain_dof[root])
      const int nchain = E->root_chain_len;
      int chain[MAXCHAIN];
#pragma unroll
      for (int c = 0; c < MAXCHAIN; c++) chain[c] = E->root_chain[c];
      if (e < 2) {
        const int k = i % 3;
        // residual and finger-dof levers from connect_rows_local (arm link's frame, fp64): rotate to
        // the world.  Arm dofs move both anchors alike: their entry is axis x (p1 - p2), tiny.
        const float* loc = &s.qfrc_con[16 * e];
        const float* R = s.xmat[root];
        float cp[3];
        m3mulv(cp, R, loc);
        const float rk[3] = {R[3 * k], R[3 * k + 1], R[3 * k + 2]};   // e_k' R: world component k of a local vector
        s.Jr[rs][b1 - 1] += v3dot(rk, loc + 4);
        if (pb1 >= GRIP0) s.Jr[rs][pb1 - 1] += v3dot(rk, loc + 7);
        s.Jr[rs][b2 - 1] += v3dot(rk, loc + 10);
        if (pb2 >= GRIP0) s.Jr[rs][pb2 - 1] += v3dot(rk, loc + 13);
        {
          // (the loop visits the chain from the record in registers, without a trip to memory per dof)
#pragma unroll
          for (int c = 0; c < MAXCHAIN; c++) {
            if (c < nchain) {
              const int j = chain[c];
              float t[3];
              v3cross(t, s.cdof[j], cp);
              s.Jr[rs][j] += sel3(t, k);
            }
          }
        }
        pos = sel3(cp, k);
        imp_pos = v3norm(cp);
        diag = invw1 + invw2;
      } else {
        const int d1 = b1 - 1, d2 = b2 - 1;
        // (the residual of two finger angles that track each other to 1e-5 rad: evaluated on the full angles)
        const double dif64 = robot_q(s, d2) - (double)q0_2;
        pos = (float)(robot_q(s, d1) - (double)q0_1 -
                      ((double)pc[0] + dif64 * ((double)pc[1] + dif64 * ((double)pc[2] + dif64 * ((double)pc[3] + dif64 * (double)pc[4])))));
        const float dif = (float)dif64;
        const float deriv = pc[1] + dif * (2.f * pc[2] + dif * (3.f * pc[3] + dif * 4.f * pc[4]));
        s.Jr[rs][d1] += 1.f;
        s.Jr[rs][d2] -= deriv;
        imp_pos = pos;
        diag = invw1 + invw2;
      }
      keep_live(root); keep_live(pb1); keep_live(pb2); keep_live(nchain); keep_live(q0_1); keep_live(q0_2);
#pragma unroll
      for (int c = 0; c < 5; c++) keep_live(pc[c]);
#pragma unroll
      for (int c = 0; c < MAXCHAIN; c++) keep_live(chain[c]);
    } else if (i < 7 + nl) {
      rs = i;
      const int info = s.lim_info[i - 7], b = info & 0xFF, hi = (info >> 8) & 1;
      const double q = robot_q(s, b - 1);
      pos = (float)(hi ? ((double)lim_range[1] - q) : (q - (double)lim_range[0]));
      s.Jr[rs][b - 1] = hi ? -1.f : 1.f;
      imp_pos = pos;
      diag = invw1;
    } else {
      const int c = (i - 7 - nl) / 3, r = (i - 7 - nl) % 3;
      const int b1 = s.con_b1[c], b2 = s.con_b2[c];
      const float* ax = &s.con_frame[c][3 * r];
      const float* p = s.con_pos[c];
      const int rs0 = s.con_rslot[c];
      if (rs0 != HDR_NONE) rs = rs0 + r;
      int slot = 0;
      float dg = 0.f;
      if (b1 > 0) {
        if (b1 < NRB) { jac_robot(M, s, rs, b1, p, ax, -1.f); dg += invw1; }
        else { pa = b1 - NRB; jac_prop(s, i, slot++, b1, p, ax, -1.f); dg += 1.0f / s.prop_mass[pa]; }
      }
      if (b2 > 0) {
        if (b2 < NRB) { jac_robot(M, s, rs, b2, p, ax, 1.f); dg += invw2; }
        else {
          const int pid = b2 - NRB;
          if (slot == 0) pa = pid; else pb = pid;
          jac_prop(s, i, slot++, b2, p, ax, 1.f);
          dg += 1.0f / s.prop_mass[pid];
        }
      }
      diag = dg;
      margin = rec_margin - rec_gap;
      imp_pos = s.con_dist[c];
      if (r == 0) pos = s.con_dist[c];
      else {
        fric_row = true;
        pos = 0.f;
        // R1 = R0/impratio ; R2 = R1 * mu0^2/mu1^2 (mu0 == mu1 for condim 3)
        R0scale = 1.0f / fmaxf(opt_impratio, kMinVal);
      }
      if (opt_cone == 0) {
        // Pyramidal cone (mj_instantiateContact / mj_makeImpedance): MuJoCo's four rows are the edges
        // n +- mu t_k, each with the contact's distance, margin and impedance, diagApprox = tran (1 + mu^2) and
        // one regulariser Rpy = 2 (mu^2 / impratio) R0.  Every edge is a combination of the three rows kept here:
        // J_e = J_n +- mu J_tk, and aref_e = aref_n +- mu aref_tk exactly (the friction rows carry K = 0 and the
        // same B and impedance), so jar_e = jar_n +- mu jar_tk: the edges are never stored, the solvers evaluate
        // the pyramid's cost on the three rows (mre_newton.h: nw_pyramid; PGS: the edge updates of a contact
        // block).  All three rows carry Rpy.
        const float fr = rec_friction;
        diag = dg * (1.f + fr * fr);
        R0scale = 2.f * fr * fr / fmaxf(opt_impratio, kMinVal);
      }
    }
    keep_live(lim_range[0]); keep_live(lim_range[1]); keep_live(invw1); keep_live(invw2); keep_live(rec_friction);
    keep_live(rec_margin); keep_live(rec_gap); keep_live(opt_impratio); keep_live(opt_cone);
    s.hdr[i] = rs | (pa << 8) | (pb << 12);
    // impedance of the block's leading row, stiffness / damping from solref
    const float imp = impedance(solimp, imp_pos, margin);
    float tc = solref[0];
    const float dr = solref[1], dmax = clampf(solimp[1], 0.0001f, 0.9999f);
    float K, B;
    if (tc > 0.f) {
      tc = fmaxf(tc, 2.f * opt_timestep);
      K = 1.0f / (dmax * dmax * tc * tc * dr * dr);
      B = 2.0f / (dmax * tc);
    } else { K = -tc / (dmax * dmax); B = -dr / dmax; }
    if (fric_row) K = 0.f;
    float R = fmaxf((1.f - imp) * diag / imp, kMinVal) * R0scale;
    if (opt_cone == 0) R = fmaxf(R, kMinVal);
    // reference acceleration (mj_referenceConstraint)
    const float vel = row_dot(s, i, s.qvel);
    const float efc_margin = fric_row ? 0.f : margin;
    const float aref = -B * vel - K * imp * (pos - efc_margin);
    rowR(s, i) = R; rowB(s, i) = aref;
#ifdef MRE_NEWTON
    if (i >= 7 + nl && (i - 7 - nl) % 3 == 0) s.con_fric[(i - 7 - nl) / 3] = rec_friction;
#else
    if (i >= 7 + nl && (i - 7 - nl) % 3 == 0) s.blkrec[8 + (i - 7 - nl) / 3][15] = rec_friction;
#endif
  }
  MRE_SYNC();
}

#ifndef MRE_NEWTON
// second half of the assembly, after the kernel body has run solve_robot_rows (Br = M^-1 Jr'); the
// phases do not nest calls, so none of them needs a callee-saved register (= scratch) to keep
// state across one
MRE_PHASE_FN void assemble_blocks(ModelP M, Sm& s, int l) {
  const int nefc = s.nefc, nl = s.nl;
  // ---- diagonal blocks of A = J M^-1 J' + R.  Contacts: 3x3 block of the contact's rows.
  // Scalar rows (equality / limit, robot-only) are grouped in consecutive triples whose
  // 3x3 block lets one solver step apply the three sequential scalar updates exactly.
  for (int i = l; i < nefc; i += 64) {
    const int h = s.hdr[i];
    const int rs = h & 0xFF, pa = (h >> 8) & 0xF, pb = (h >> 12) & 0xF;
    const bool scalar = i < 7 + nl;
    const int r = scalar ? i % 3 : (i - 7 - nl) % 3;
    const int i0 = i - r;
    const int nb = scalar ? ((7 + nl - i0) < 3 ? (7 + nl - i0) : 3) : 3;
    const int slot = scalar ? i / 3 : 8 + (i - 7 - nl) / 3;
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
      float a = 0.f;
      if (cc < nb) {
        if (rs != HDR_NONE) {
          const int rs2 = rs - r + cc;
          for (int j = 0; j < NRV; j++) a += s.Jr[rs][j] * s.Br[rs2][j];
        }
        if (pa < NPROP)
          { const float *x = jpA(s, i), *y = jpA(s, i0 + cc); for (int k = 0; k < 6; k++) a += x[k] * y[k] * prop_invM(s, pa, k); }
        if (pb < NPROP)
          { const float *x = jpB(s, i), *y = jpB(s, i0 + cc); for (int k = 0; k < 6; k++) a += x[k] * y[k] * prop_invM(s, pb, k); }
      }
      acc[cc] = a;
    }
    const float diag = (r == 0 ? acc[0] : (r == 1 ? acc[1] : acc[2])) + rowR(s, i);
    if (r == 0) acc[0] = scalar ? acc[0] : diag;
    if (r == 1) acc[1] = scalar ? acc[1] : diag;
    if (r == 2) acc[2] = scalar ? acc[2] : diag;
    // symmetric block, upper triangle packed as (00,01,02,11,12,22) -- like the mirrored AR of mj_projectConstraint
    if (r == 0) { s.blkrec[slot][9] = acc[0]; s.blkrec[slot][10] = acc[1]; s.blkrec[slot][11] = acc[2]; }
    if (r == 1) { s.blkrec[slot][12] = acc[1]; s.blkrec[slot][13] = acc[2]; }
    if (r == 2) { s.blkrec[slot][14] = acc[2]; }
    s.blkrec[slot][6 + r] = 1.0f / diag;
  }
  MRE_SYNC();
}

MRE_DEV float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// mju_QCQP2
MRE_DEV bool qcqp2(float* res, const float* A, const float* b, float d0, float d1, float r) {
  const float b1 = b[0] * d0, b2 = b[1] * d1;
  const float A11 = A[0] * d0 * d0, A22 = A[3] * d1 * d1, A12 = A[1] * d0 * d1;
  float la = 0.f, v1 = 0.f, v2 = 0.f;
  const float r2 = r * r;
  for (int iter = 0; iter < 20; iter++) {
    const float det = (A11 + la) * (A22 + la) - A12 * A12;
    if (det < 1e-10f) { res[0] = res[1] = 0.f; return false; }
    const float di = fast_rcp(det);
    const float P11 = (A22 + la) * di, P22 = (A11 + la) * di, P12 = -A12 * di;
    v1 = -P11 * b1 - P12 * b2;
    v2 = -P12 * b1 - P22 * b2;
    const float val = v1 * v1 + v2 * v2 - r * r;
    // mju_QCQP2 stops at val < 1e-10; in fp32 |v|^2 - r^2 cannot be resolved below ~1e-7 r^2, so a
    // sliding contact would spin through all 20 Newton steps on rounding noise: stop at fp32
    // resolution instead (the caller rescales v onto the cone exactly afterwards)
    if (val < fmaxf(1e-10f, 1e-6f * r2)) break;
    const float deriv = -2.0f * (P11 * v1 * v1 + 2.0f * P12 * v1 * v2 + P22 * v2 * v2);
    const float delta = -val * fast_rcp(deriv);
    if (delta < 1e-10f) break;
    la += delta;
  }
  res[0] = v1 * d0;
  res[1] = v2 * d1;
  return la != 0.f;
}

// ---------------------------------------------------------------------------
// Solver lane layout: lanes 0..14 = robot dofs (DPP row 0), lanes 16+8p+k (k<6) =
// dof k of cube p (one 8-lane half-row per cube).  Islands: 0 = robot, 1+p = cube p.
MRE_DEV int lane_island(int l) { return l < 16 ? 0 : (l < 48 ? 1 + ((l - 16) >> 3) : -1); }
MRE_DEV int lane_dof(int l) {
  if (l < NRV) return l;
  if (l >= 16 && l < 48 && ((l - 16) & 7) < 6) return NRV + 6 * ((l - 16) >> 3) + ((l - 16) & 7);
  return -1;
}
// sums over the lanes of one island (8-lane halves everywhere, full 16 lanes on DPP row 0),
// three island sums at once
MRE_DEV void island_sum3(float& x, float& y, float& z) {
  // one v_add_f32_dpp per value and level; the three chains interleave, which also provides the
  // two wait states a DPP read needs after the VALU write of its source (s_nop covers the entry).
  // The last level runs on DPP row 0 only: the other rows keep their 8-lane sums.
  asm volatile(
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_add_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_add_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_add_f32_dpp %2, %2, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_add_f32_dpp %1, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_add_f32_dpp %2, %2, %2 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_add_f32_dpp %0, %0, %0 row_mirror row_mask:0x1 bank_mask:0xf\n\t"
      "v_add_f32_dpp %1, %1, %1 row_mirror row_mask:0x1 bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %2, %2 row_mirror row_mask:0x1 bank_mask:0xf\n\t"
      "s_nop 1"
      : "+v"(x), "+v"(y), "+v"(z));
}

// J / B entry of row `row` for the dof this lane owns (rs = robot slot or NONE, slot = which
// prop part of the row belongs to this lane's cube)
MRE_DEV void lane_JB(const Sm& s, int row, int rs, int l, int lk, int slot, float linvM, float& j, float& b) {
  j = 0.f; b = 0.f;
  if (l < NRV) {
    if (rs != BLK_NONE) { j = s.Jr[rs][l]; b = s.Br[rs][l]; }
  } else if (slot >= 0) {
    j = (slot == 0 ? jpA(s, row) : jpB(s, row))[lk];
    b = j * linvM;
  }
}

// (block descriptor: struct Blk, declared next to struct Sm)

// Build the block list (global MuJoCo row order) and its ASAP schedule: block b runs at
// step 1 + max(last step of every island it touches).  Blocks of one step touch disjoint
// islands, and any two blocks sharing an island keep their sequential order, so a sweep over
// the schedule produces exactly the iterates of the sequential Gauss-Seidel sweep.
MRE_DEV void build_schedule(ModelP M, Sm& s) {
  int* last = s.iscr;  // per-island last step (LDS; lane 0 only)
  for (int k = 0; k < 5; k++) last[k] = 0;
  const int nscalar = 7 + s.nl;
  int nb = 0, nst = 0;
  // (every entry of s.sched was set to SCHED_NONE by the whole wave before this lane-0 routine)
  for (int i = 0; i < nscalar; i += 3) {
    Blk b;
    b.row0 = (uint16_t)i; b.type = 0; b.nrows = (uint8_t)((nscalar - i) < 3 ? (nscalar - i) : 3);
    b.rslot = (uint8_t)i; b.pa = 0xF; b.pb = 0xF; b.primary = 0; b.bslot = 0;
    const int st = last[0]++;
    s.sched[st][0] = (uint8_t)nb;
    s.blk[nb++] = b;
    if (last[0] > nst) nst = last[0];
  }
  for (int c = 0; c < s.ncon; c++) {
    const int b1 = s.con_b1[c], b2 = s.con_b2[c];
    const int rs = s.con_rslot[c];
    int pa = 0xF, pb = 0xF;
    if (b1 >= NRB) pa = b1 - NRB;
    if (b2 >= NRB) { if (pa == 0xF) pa = b2 - NRB; else pb = b2 - NRB; }
    const bool hr = rs != HDR_NONE, ha = pa != 0xF, hb = pb != 0xF;
    int st = 0;
    if (hr && last[0] > st) st = last[0];
    if (ha && last[1 + pa] > st) st = last[1 + pa];
    if (hb && last[1 + pb] > st) st = last[1 + pb];
    Blk b;
    b.row0 = (uint16_t)(nscalar + 3 * c); b.type = 2; b.nrows = 3;
    b.rslot = (uint8_t)(hr ? rs : BLK_NONE); b.pa = (uint8_t)pa; b.pb = (uint8_t)pb;
    b.primary = (uint8_t)(hr ? 0 : 1 + pa); b.bslot = (uint8_t)(hb ? s.con_bslot[c] : 0);
    if (hr) { last[0] = st + 1; s.sched[st][0] = (uint8_t)nb; }
    if (ha) { last[1 + pa] = st + 1; s.sched[st][1 + pa] = (uint8_t)nb; }
    if (hb) { last[1 + pb] = st + 1; s.sched[st][1 + pb] = (uint8_t)nb; }
    if (st + 1 > nst) nst = st + 1;
    s.blk[nb++] = b;
  }
  s.nblk = nb;
  s.nsched = nst;
}

// ------------------------------------------------------------- mj_fwdConstraint
// On exit: s.qacc = qacc_smooth + M^-1 J' f, s.qfrc_con = J' f.
// PYR: pyramidal friction cones (opt.cone == 0); the two instantiations are separate phase functions, so the
// elliptic one carries nothing of the other
template <bool PYR>
MRE_DEV void solve_constraints_impl(ModelP M, Sm& s, int l) {
  const int nefc = s.nefc, nl = s.nl;
  const int isl = lane_island(l);
  const int ldof = lane_dof(l);
  const int lp = (isl > 0) ? isl - 1 : -1;
  const int lk = (isl > 0) ? ((l - 16) & 7) : 0;
  const bool lvalid = ldof >= 0;
  const float linvM = (lp >= 0 && lvalid) ? prop_invM(s, lp, lk) : 0.f;
  const bool leader = (l == 0) || (l >= 16 && l < 48 && lk == 0);
  float* jar = s.jar;
  // Pyramidal cones (opt.cone): MuJoCo's PGS walks the four edge rows e = n +- mu t_k of a contact as scalar
  // one-sided rows with one regulariser Rpy.  The edges are combinations of the contact's three rows
  // (assemble_constraints), so a contact stays ONE block: its residual J a + b and its 3 x 3 block of J M^-1 J' are
  // those of the three rows, the four sequential edge updates run inside the block step on them, and the edge
  // forces (pyr_f) are kept beside their image f = E' f_e that everything outside the block sees.
  constexpr bool pyr = PYR;
  // ---- efc_b and warm-start forces (mj_constraintUpdate on J*qacc_warmstart - aref)
  for (int i = l; i < nefc; i += 64) {
    const float aref = rowB(s, i);
    float d1, d2;
    row_dot2(s, i, s.qacc, s.qacc_smooth, d1, d2);
    jar[i] = d1 - aref;
    rowB(s, i) = d2 - aref;
  }
  MRE_SYNC();
  for (int i = l; i < nefc; i += 64) {
    const float D = 1.0f / rowR(s, i);
    if (i < 7) s.frc[i] = -D * jar[i];
    else if (i < 7 + nl) s.frc[i] = jar[i] < 0.f ? -D * jar[i] : 0.f;
    else if ((i - 7 - nl) % 3 == 0) {
      const int c = (i - 7 - nl) / 3;
      const float fr0 = s.blkrec[8 + c][15];
      if (pyr) {
        const float j0 = jar[i], j1 = fr0 * jar[i + 1], j2 = fr0 * jar[i + 2];
        const float g0 = -D * fminf(j0 + j1, 0.f), g1 = -D * fminf(j0 - j1, 0.f);
        const float g2 = -D * fminf(j0 + j2, 0.f), g3 = -D * fminf(j0 - j2, 0.f);
        s.pyr_f[4 * c] = g0; s.pyr_f[4 * c + 1] = g1; s.pyr_f[4 * c + 2] = g2; s.pyr_f[4 * c + 3] = g3;
        s.frc[i] = (g0 + g1) + (g2 + g3); s.frc[i + 1] = fr0 * (g0 - g1); s.frc[i + 2] = fr0 * (g2 - g3);
        continue;
      }
      const float D1 = 1.0f / rowR(s, i + 1), D2 = 1.0f / rowR(s, i + 2);
      const float mu = fr0 * sqrtf(rowR(s, i + 1) / rowR(s, i));
      const float j0 = jar[i], j1 = jar[i + 1], j2 = jar[i + 2];
      const float U0 = j0 * mu, U1 = j1 * fr0, U2 = j2 * fr0;
      const float N = U0, T = sqrtf(U1 * U1 + U2 * U2);
      float f0, f1, f2;
      // top zone (jar in the polar cone): no force; bottom zone (-D*jar inside the friction cone)
      if (N >= mu * T || (T <= 0.f && N >= 0.f)) { f0 = f1 = f2 = 0.f; }
      else if (mu * N + T <= 0.f || (T <= 0.f && N < 0.f)) { f0 = -D * j0; f1 = -D1 * j1; f2 = -D2 * j2; }
      else {
        const float Dm = D / fmaxf(mu * mu * (1.f + mu * mu), kMinVal);
        const float NT = N - mu * T;
        f0 = -Dm * NT * mu;
        f1 = -f0 / T * U1 * fr0;
        f2 = -f0 / T * U2 * fr0;
      }
      s.frc[i] = f0; s.frc[i + 1] = f1; s.frc[i + 2] = f2;
    }
  }
  // (elliptic cones: pyr_f carries the low-order words of the forces of robot contacts, see the block step)
  if (!pyr) for (int i = l; i < 4 * s.ncon; i += 64) s.pyr_f[i] = 0.f;
  MRE_SYNC();
  // ---- a = M^-1 J' f, w = J' f for the warm start (lane = dof in the solver layout)
  float a = 0.f, w = 0.f;
  for (int bi = 0; bi < s.nblk; bi++) {
    const Blk bk = s.blk[bi];
    const int row0 = bk.row0, rs = bk.rslot, nr = bk.nrows;
    const int slot = (lp >= 0 && lvalid) ? (lp == bk.pa ? 0 : (lp == bk.pb ? 1 : -1)) : -1;
    for (int r = 0; r < nr; r++) {
      const float fi = s.frc[row0 + r];
      float j, b;
      lane_JB(s, row0 + r, rs == BLK_NONE ? BLK_NONE : rs + r, l, lk, slot, linvM, j, b);
      a += b * fi;
      w += j * fi;
    }
  }
  if (l < NVP) s.scratch[l] = 0.f;
  MRE_SYNC();
  if (lvalid) s.scratch[ldof] = a;
  MRE_SYNC();
  // dual cost 0.5 f'ARf + f'b ; cold start if positive
  float part = 0.f;
  for (int i = l; i < nefc; i += 64) {
    const float fi = s.frc[i];
    const bool prow = pyr && i >= 7 + nl;   // the regulariser acts on the edge forces, not on their image
    const float Af = row_dot(s, i, s.scratch) + (prow ? 0.f : rowR(s, i) * fi);
    part += fi * (0.5f * Af + rowB(s, i));
    if (prow && (i - 7 - nl) % 3 == 0) {
      const float* g = &s.pyr_f[4 * ((i - 7 - nl) / 3)];
      part += 0.5f * rowR(s, i) * ((g[0] * g[0] + g[1] * g[1]) + (g[2] * g[2] + g[3] * g[3]));
    }
  }
  const float cost = wave_sum(part);
  MRE_SYNC();
  if (cost > 0.f) {
    a = 0.f; w = 0.f;
    for (int i = l; i < nefc; i += 64) s.frc[i] = 0.f;
    if (pyr) for (int i = l; i < 4 * s.ncon; i += 64) s.pyr_f[i] = 0.f;
  }
  MRE_SYNC();
  // ---- PGS sweeps over the island schedule
  const int nva = NRV + 6 * s.nprops;
  float msum = M->opt_rec.M0_diag_robot_sum;
  for (int p = 0; p < s.nprops; p++)
    msum += 3.f * s.prop_mass[p] + s.prop_inertia[p][0] + s.prop_inertia[p][1] + s.prop_inertia[p][2];
  const float scale = 1.0f / ((msum / nva) * nva);
  // (wave-uniform by construction; said so, the step counters of the sweep live in scalar registers)
  const int nsched = __builtin_amdgcn_readfirstlane(s.nsched), max_iter = M->opt_rec.iterations, nscalar = 7 + nl;
  const float tol = M->opt_rec.tolerance;
  // Operand table: the schedule's descriptor words expanded once per solve into LDS byte offsets,
  // so that a sweep step costs one 8-byte read per lane instead of a decode.  It lives in the
  // body-frame arrays and region R1, which nothing reads between the controller and the next
  // position stage.  Entry (step, island):
  //   x = offset of the island's first Jacobian row | offset of the block record << 16
  //   y = row0 | nrows << 8 | on << 10 | contact << 11 | primary << 12 | partner lane << 13 | coupled << 19 |
  //       robot contact << 20
  static_assert(offsetof(Sm, xpos) % 8 == 0 &&
                offsetof(Sm, cdof) - offsetof(Sm, xpos) >= sizeof(uint2) * (TAB_OFF + 1) + sizeof(float) * TAB_ZEROS,
                "operand table must fit in the body-frame arrays + region R1");
  static_assert(TAB_ZEROS * 4 >= 4 * (NRV - 1) + 2 * 4 * NRV + 4, "zero pad covers three robot rows");
  char* const sb = reinterpret_cast<char*>(&s);
  uint2* const tab = reinterpret_cast<uint2*>(&s.xpos[0][0]);
  float* const zeros = reinterpret_cast<float*>(tab + TAB_OFF + 1);
  for (int e = l; e < nsched * 5; e += 64) {
    const int st = e / 5, is = e - 5 * st;
    const int bi = s.sched[st][is];
    const bool on = bi != SCHED_NONE;
    const Blk bk = s.blk[on ? bi : 0];
    const int type = bk.type, row0 = on ? bk.row0 : 0, rs = bk.rslot, nr = on ? bk.nrows : 0;
    const int pa = bk.pa, pb = bk.pb, ip = is - 1;
    const bool is3 = on && type == 2;
    int partner = 0, coupled = 0;
    if (is3) {
      if (is == 0) { if (pa != 0xF) { partner = 16 + 8 * pa; coupled = 1; } }
      else if (rs != BLK_NONE) { partner = 0; coupled = 1; }
      else if (pb != 0xF) { partner = 16 + 8 * (ip == pa ? pb : pa); coupled = 1; }
    }
    const float* jrow = zeros;
    if (on) jrow = (is == 0) ? &s.Jr[rs][0] : (ip == pa ? &s.JpA[row0 - nscalar][0] : &s.JpB[3 * bk.bslot][0]);
    const int bidx = is3 ? 8 + (row0 - nscalar) / 3 : row0 / 3;
    const unsigned joff = (unsigned)(reinterpret_cast<const char*>(jrow) - sb);
    const unsigned roff = (unsigned)(reinterpret_cast<const char*>(s.blkrec[on ? bidx : 0]) - sb);
    uint2 ent;
    ent.x = joff | (roff << 16);
    ent.y = (unsigned)row0 | ((unsigned)nr << 8) | ((unsigned)on << 10) | ((unsigned)is3 << 11) |
            ((unsigned)(on && is == bk.primary) << 12) | ((unsigned)partner << 13) | ((unsigned)coupled << 19) |
            ((unsigned)(is3 && rs != BLK_NONE) << 20);   // bit 20: a contact with a robot part (fp64 block update)
    tab[e] = ent;
  }
  if (l == 63) {
    uint2 ent;
    ent.x = (unsigned)(reinterpret_cast<const char*>(zeros) - sb) | ((unsigned)(reinterpret_cast<const char*>(s.blkrec[0]) - sb) << 16);
    ent.y = 0u;
    tab[TAB_OFF] = ent;
  }
  if (l < TAB_ZEROS) zeros[l] = 0.f;
  MRE_SYNC();
  // per-lane constants: lanes that own no dof read the all-off entry at every step
  const bool rob_lane = l < NRV;
  const unsigned tab0 = (unsigned)(reinterpret_cast<const char*>(tab) - sb);
  const unsigned tbase = tab0 + 8u * (lvalid ? (unsigned)isl : (unsigned)TAB_OFF);
  const unsigned tstep = lvalid ? 40u : 0u;
  const unsigned loff = 4u * (rob_lane ? (unsigned)l : (unsigned)lk);
  const unsigned lstr = rob_lane ? 4u * NRV : 24u;
  const unsigned broff = (unsigned)(reinterpret_cast<const char*>(&s.Br[0][0]) - reinterpret_cast<const char*>(&s.Jr[0][0]));
  const float* const frc = s.frc;
  int iters = 0;
  // The operands of a step that no step writes (schedule entry, Jacobian / M^-1 J' rows, block record)
  // are fetched one step ahead, so that their two dependent LDS round trips overlap the block update
  // of the current step instead of stalling the next one (2 waves per SIMD hide little by themselves).
  struct StepOps { uint2 ent; float j0, j1r, j2r, b0r, b1r, b2r; float4 q0, q1, q2, q3; };
  auto fetch_ent = [&](int st) { return *reinterpret_cast<const uint2*>(sb + tbase + tstep * (unsigned)st); };
  auto fetch_rows = [&](uint2 ent) {
    StepOps o;
    o.ent = ent;
    // three rows through the lane's offset / stride (rows past the block may hold stale non-finite
    // LDS contents: select, never multiply by zero)
    const char* jp = sb + ((ent.x & 0xFFFFu) + loff);
    o.j0 = *reinterpret_cast<const float*>(jp);
    o.j1r = *reinterpret_cast<const float*>(jp + lstr);
    o.j2r = *reinterpret_cast<const float*>(jp + 2u * lstr);
    o.b0r = *reinterpret_cast<const float*>(jp + broff);
    o.b1r = *reinterpret_cast<const float*>(jp + lstr + broff);
    o.b2r = *reinterpret_cast<const float*>(jp + 2u * lstr + broff);
    // the block's uniform operands: one 64-byte record, four 16-byte LDS reads
    // (explicit LDS address space: the generic pointer hides the record's 16-byte alignment from the compiler,
    //  which then splits each 16-byte read in two)
    typedef float rec4 __attribute__((ext_vector_type(4)));
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(3))) rec4* rec = (const __attribute__((address_space(3))) rec4*)(sb + (ent.x >> 16));
#else
    const rec4* rec = reinterpret_cast<const rec4*>(sb + (ent.x >> 16));
#endif
    const rec4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    o.q0 = make_float4(r0.x, r0.y, r0.z, r0.w); o.q1 = make_float4(r1.x, r1.y, r1.z, r1.w);
    o.q2 = make_float4(r2.x, r2.y, r2.z, r2.w); o.q3 = make_float4(r3.x, r3.y, r3.z, r3.w);
    return o;
  };
  int st = 0, iter = 0;
  float impr = 0.f;
  uint2 ent1 = fetch_ent(nsched > 1 ? 1 : 0);   // schedule entry of the step after the next fetch
  // one schedule step on the operands `cur`; the operands of the following step go to `nxt`.  The
  // loop below calls it with two operand sets in turn (no register shuffling between steps).
  // Returns true when the solve is over.
  auto step = [&](const StepOps& cur, StepOps& nxt) -> bool {
      const int st1 = st + 1 < nsched ? st + 1 : 0;
      const int st2 = st1 + 1 < nsched ? st1 + 1 : 0;
      nxt = fetch_rows(ent1);
      ent1 = fetch_ent(st2);
      const uint2 ent = cur.ent;
      const unsigned w1 = ent.y;
      const bool on = (w1 & 0x400u) != 0u, is3 = (w1 & 0x800u) != 0u;
      const int row0 = (int)(w1 & 0xFFu), nr = (int)((w1 >> 8) & 3u);
      const bool h1 = nr > 1, h2 = nr > 2;
      const float j0 = cur.j0, j1r = cur.j1r, j2r = cur.j2r, b0r = cur.b0r, b1r = cur.b1r, b2r = cur.b2r;
      const float j1 = h1 ? j1r : 0.f, j2 = h2 ? j2r : 0.f;
      const float b1 = h1 ? b1r : 0.f, b2 = h2 ? b2r : 0.f;
      const float4 q0 = cur.q0, q1 = cur.q1, q2 = cur.q2, q3 = cur.q3;
      const float4 r0 = make_float4(q0.x, q0.w, 0.f, q1.z);
      const float4 r1 = make_float4(q0.y, q1.x, 0.f, q1.w);
      const float4 r2 = make_float4(q0.z, q1.y, 0.f, q2.x);
      const float f0 = frc[row0], f1r = frc[row0 + 1], f2r = frc[row0 + 2];
      const float f1 = h1 ? f1r : 0.f, f2 = h2 ? f2r : 0.f;
      float p0 = j0 * a, p1 = j1 * a, p2 = j2 * a;
      island_sum3(p0, p1, p2);
      if (__any((w1 & 0x80000u) != 0u)) {
        const int src = (int)((w1 >> 11) & 0xFCu);  // partner lane * 4
        const float x0 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, p0)));
        const float x1 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, p1)));
        const float x2 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, p2)));
        if ((w1 & 0x80000u) != 0u) { p0 += x0; p1 += x1; p2 += x2; }
      }
      float d0 = 0.f, d1 = 0.f, d2 = 0.f, change = 0.f;
      float nh0 = 0.f, nh1 = 0.f, nh2 = 0.f;   // the new forces as stored (set by the fp64 branch only)
#ifdef MRE_PGS_F32   // (A/B builds, tools/build_variant.py: every block update in float32, as up to round 3)
      const bool rob3 = false;
#else
      const bool rob3 = !pyr && (w1 & 0x100000u) != 0u;
#endif
      if (on) {
        const float A00 = q2.y, A01 = q2.z, A02 = q2.w, A11 = q3.x, A12 = q3.y, A22 = q3.z;
        const float A10 = A01, A20 = A02, A21 = A12;
        const float res0 = p0 + r0.x * f0 + r0.y, res1 = p1 + r1.x * f1 + r1.y, res2 = p2 + r2.x * f2 + r2.y;
        if (!is3) {
          // up to three sequential scalar updates; cross terms through the block's A entries.
          // Rows past nr are neutralised with selects (no divergent branches in this path).
          float fn = f0 - res0 * r0.w;
          fn = (row0 >= 7 && fn < 0.f) ? 0.f : fn;
          d0 = fn - f0;
          float ch0 = d0 * (0.5f * d0 * (A00 + r0.x) + res0);
          d0 = ch0 > 1e-10f ? 0.f : d0;
          ch0 = ch0 > 1e-10f ? 0.f : ch0;
          const float rs1 = res1 + A10 * d0;
          fn = f1 - rs1 * r1.w;
          fn = (row0 + 1 >= 7 && fn < 0.f) ? 0.f : fn;
          d1 = h1 ? fn - f1 : 0.f;
          float ch1 = d1 * (0.5f * d1 * (A11 + r1.x) + rs1);
          d1 = ch1 > 1e-10f ? 0.f : d1;
          ch1 = ch1 > 1e-10f ? 0.f : ch1;
          const float rs2 = res2 + A20 * d0 + A21 * d1;
          fn = f2 - rs2 * r2.w;
          fn = (row0 + 2 >= 7 && fn < 0.f) ? 0.f : fn;
          d2 = h2 ? fn - f2 : 0.f;
          float ch2 = d2 * (0.5f * d2 * (A22 + r2.x) + rs2);
          d2 = ch2 > 1e-10f ? 0.f : d2;
          ch2 = ch2 > 1e-10f ? 0.f : ch2;
          change = ch0 + ch1 + ch2;
        } else if (pyr) {
          // four sequential scalar updates on the edges (1, +-fr, 0), (1, 0, +-fr); g = J a + b on the three rows
          // follows every update through the block's J M^-1 J' (the record's A carries Rpy on its diagonal)
          const float fr = q3.w, Rp = r0.x;
          const float B00 = A00 - Rp, B11 = A11 - Rp, B22 = A22 - Rp;
          float g0 = p0 + r0.y, g1 = p1 + r1.y, g2 = p2 + r2.y;
          float* const fe = &s.pyr_f[4 * ((row0 - nscalar) / 3)];
          float e0 = fe[0], e1 = fe[1], e2 = fe[2], e3 = fe[3];
          auto edge1 = [&](float& f, float sf) {
            const float res = g0 + sf * g1 + Rp * f;
            const float AR = B00 + 2.f * sf * A01 + sf * sf * B11 + Rp;
            float d = fmaxf(f - res * fast_rcp(AR), 0.f) - f;
            float ch = d * (0.5f * d * AR + res);
            if (ch > 1e-10f) { d = 0.f; ch = 0.f; }
            g0 += (B00 + sf * A01) * d; g1 += (A01 + sf * B11) * d; g2 += (A02 + sf * A12) * d;
            f += d; change += ch;
          };
          auto edge2 = [&](float& f, float sf) {
            const float res = g0 + sf * g2 + Rp * f;
            const float AR = B00 + 2.f * sf * A02 + sf * sf * B22 + Rp;
            float d = fmaxf(f - res * fast_rcp(AR), 0.f) - f;
            float ch = d * (0.5f * d * AR + res);
            if (ch > 1e-10f) { d = 0.f; ch = 0.f; }
            g0 += (B00 + sf * A02) * d; g1 += (A01 + sf * A12) * d; g2 += (A02 + sf * B22) * d;
            f += d; change += ch;
          };
          edge1(e0, fr); edge1(e1, -fr); edge2(e2, fr); edge2(e3, -fr);
          d0 = ((e0 + e1) + (e2 + e3)) - f0; d1 = fr * (e0 - e1) - f1; d2 = fr * (e2 - e3) - f2;
          if (leader) { fe[0] = e0; fe[1] = e1; fe[2] = e2; fe[3] = e3; }
        } else if (rob3) {
          // A contact that touches the robot: the same update in fp64 on the same float32 operands, the force kept
          // as a float32 pair (frc + its low-order word in pyr_f, which elliptic cones leave free).
          // Why: PGS stops at its sweep cap, not at the optimum, so the iterate itself has to be reproduced.  A float32
          // force of 100 N moves in steps of 8e-6 N; through M^-1 J' that is 1e-3 rad/s^2 on the few-gram finger links
          // the arm carries, every sweep, and no later stage can take it back.  CPU study (the fp64 oracle running
          // this matrix-free sweep with float32 roundings, tests/diagnostics/pgs_precision_study.py): everything float32
          // leaves the 1e-4 bar in the envs the device left it in (21, 33, 34 of the 64-env bench law); with the force,
          // residual and update of ROBOT CONTACT rows in double -- accumulators, Jacobians, M^-1 J', diagonal blocks and
          // every other row still float32 -- 64 of 64 stay within 3e-5 (scalar rows alone in double: no change).
          // (Measured on the device too, round 4: the scalar rows' updates in fp64 as well cost 19 % of the PGS tick --
          //  a dependent chain of thirty fp64 operations per step -- and moved the 256-env sample from 249 to 250.)
          const int cix = (row0 - nscalar) / 3;
          float* const flo = &s.pyr_f[4 * cix];
          const double F0 = (double)f0 + (double)flo[0], F1 = (double)f1 + (double)flo[1], F2 = (double)f2 + (double)flo[2];
          const double a00 = A00, a01 = A01, a02 = A02, a11 = A11, a12 = A12, a22 = A22;
          const double e0 = (double)p0 + (double)r0.x * F0 + (double)r0.y, e1 = (double)p1 + (double)r1.x * F1 + (double)r1.y,
                       e2 = (double)p2 + (double)r2.x * F2 + (double)r2.y;
          const double fr = q3.w;
          double n0 = F0, n1 = F1, n2 = F2;
          if (n0 < (double)kMinVal) {
            n0 -= e0 * rcp64(a00);
            if (n0 < 0.0) n0 = 0.0;
            n1 = n2 = 0.0;
          } else {
            const double v0 = a00 * n0 + a01 * n1 + a02 * n2, v1 = a01 * n0 + a11 * n1 + a12 * n2,
                         v2 = a02 * n0 + a12 * n1 + a22 * n2;
            const double denom = n0 * v0 + n1 * v1 + n2 * v2;
            if (denom >= (double)kMinVal) {
              double x = -(n0 * e0 + n1 * e1 + n2 * e2) * rcp64(denom);
              if (n0 + x * n0 < 0.0) x = -1.0;
              n0 += x * F0; n1 += x * F1; n2 += x * F2;
            }
          }
          const double bc0 = e1 - a11 * F1 - a12 * F2 + a01 * (n0 - F0), bc1 = e2 - a12 * F1 - a22 * F2 + a02 * (n0 - F0);
          if (n0 < (double)kMinVal) {
            n1 = n2 = 0.0;
          } else {
            // mju_QCQP2 (d0 = d1 = fr, r = n0)
            const double b1 = bc0 * fr, b2 = bc1 * fr, fr2 = fr * fr;
            const double Q11 = a11 * fr2, Q22 = a22 * fr2, Q12 = a12 * fr2;
            double la = 0.0, u1 = 0.0, u2 = 0.0;
            bool ok = true;
            for (int it = 0; it < 20; it++) {
              const double det = (Q11 + la) * (Q22 + la) - Q12 * Q12;
              if (det < 1e-10) { ok = false; break; }
              const double di = rcp64(det);
              const double P11 = (Q22 + la) * di, P22 = (Q11 + la) * di, P12 = -Q12 * di;
              u1 = -P11 * b1 - P12 * b2;
              u2 = -P12 * b1 - P22 * b2;
              const double val = u1 * u1 + u2 * u2 - n0 * n0;
              if (val < 1e-10) break;
              const double deriv = -2.0 * (P11 * u1 * u1 + 2.0 * P12 * u1 * u2 + P22 * u2 * u2);
              const double delta = -val * rcp64(deriv);
              if (delta < 1e-10) break;
              la += delta;
            }
            if (!ok) { n1 = n2 = 0.0; }
            else {
              n1 = u1 * fr; n2 = u2 * fr;
              if (la != 0.0) {
                // back onto the cone: v *= sqrt(n0^2 / sum (v_i / mu)^2)
                const double ss = u1 * u1 + u2 * u2;
                const double sc = n0 * rsq64(ss > (double)kMinVal ? ss : (double)kMinVal);   // (n0 >= kMinVal > 0 here)
                n1 *= sc; n2 *= sc;
              }
            }
          }
          double D0 = n0 - F0, D1 = n1 - F1, D2 = n2 - F2;
          const double Ad0 = a00 * D0 + a01 * D1 + a02 * D2, Ad1 = a01 * D0 + a11 * D1 + a12 * D2,
                       Ad2 = a02 * D0 + a12 * D1 + a22 * D2;
          double ch = 0.5 * (D0 * Ad0 + D1 * Ad1 + D2 * Ad2) + D0 * e0 + D1 * e1 + D2 * e2;
          if (ch > 1e-10) { D0 = D1 = D2 = 0.0; ch = 0.0; n0 = F0; n1 = F1; n2 = F2; }
          change = (float)ch;
          d0 = (float)D0; d1 = (float)D1; d2 = (float)D2;
          nh0 = (float)n0; nh1 = (float)n1; nh2 = (float)n2;
          if (leader) { flo[0] = (float)(n0 - (double)nh0); flo[1] = (float)(n1 - (double)nh1); flo[2] = (float)(n2 - (double)nh2); }
        } else {
          const float fr = q3.w;
          float n0 = f0, n1 = f1, n2 = f2;
          if (n0 < kMinVal) {
            n0 -= res0 * r0.w;  // 1/A00 (regulariser included) precomputed at assembly
            if (n0 < 0.f) n0 = 0.f;
            n1 = n2 = 0.f;
          } else {
            const float v0 = A00 * n0 + A01 * n1 + A02 * n2, v1 = A10 * n0 + A11 * n1 + A12 * n2,
                        v2 = A20 * n0 + A21 * n1 + A22 * n2;
            const float denom = n0 * v0 + n1 * v1 + n2 * v2;
            if (denom >= kMinVal) {
              float x = -(n0 * res0 + n1 * res1 + n2 * res2) * fast_rcp(denom);
              if (n0 + x * n0 < 0.f) x = -1.0f;
              n0 += x * f0; n1 += x * f1; n2 += x * f2;
            }
          }
          const float Ac[4] = {A11, A12, A21, A22};
          float bc[2];
          bc[0] = res1 - A11 * f1 - A12 * f2 + A10 * (n0 - f0);
          bc[1] = res2 - A21 * f1 - A22 * f2 + A20 * (n0 - f0);
          if (n0 < kMinVal) {
            n1 = n2 = 0.f;
          } else {
            float v[2];
            const bool active = qcqp2(v, Ac, bc, fr, fr, n0);
            if (active) {
              // put v back on the cone: v *= n0 * mu / |v|  (= sqrt(n0^2 / sum (v_i/mu)^2))
              const float sq = n0 * fr * __builtin_amdgcn_rsqf(fmaxf(v[0] * v[0] + v[1] * v[1], kMinVal));
              v[0] *= sq; v[1] *= sq;
            }
            n1 = v[0]; n2 = v[1];
          }
          d0 = n0 - f0; d1 = n1 - f1; d2 = n2 - f2;
          const float Ad0 = A00 * d0 + A01 * d1 + A02 * d2, Ad1 = A10 * d0 + A11 * d1 + A12 * d2,
                      Ad2 = A20 * d0 + A21 * d1 + A22 * d2;
          change = 0.5f * (d0 * Ad0 + d1 * Ad1 + d2 * Ad2) + d0 * res0 + d1 * res1 + d2 * res2;
          if (change > 1e-10f) { d0 = d1 = d2 = 0.f; change = 0.f; }
        }
        if ((w1 & 0x1000u) != 0u) impr -= change;
        if (leader) {
          s.frc[row0] = rob3 ? nh0 : f0 + d0;
          if (h1) s.frc[row0 + 1] = rob3 ? nh1 : f1 + d1;
          if (h2) s.frc[row0 + 2] = rob3 ? nh2 : f2 + d2;
        }
      }
      // a += B'd, w += J'd (cube lanes: B = J / M_dof; lanes of an idle island keep d = 0, and
      // their B operands are unspecified, hence the select)
      const float wu = j0 * d0 + j1 * d1 + j2 * d2;
      const float au = b0r * d0 + b1 * d1 + b2 * d2;
      a += rob_lane ? (on ? au : 0.f) : linvM * wu;
      w += wu;
      MRE_SYNC();
      st = st1;
      if (st1 != 0) return false;
      // end of a sweep
      iters = ++iter;
      const float improvement = wave_sum(leader ? impr : 0.f);
      impr = 0.f;
      return improvement * scale < tol || iter >= max_iter;
  };
  if (max_iter > 0 && nsched > 0) {
    StepOps opsA = fetch_rows(fetch_ent(0)), opsB;
    for (;;) {
      if (step(opsA, opsB)) break;
      if (step(opsB, opsA)) break;
    }
  } else if (max_iter > 0) {
    iters = 1;
  }
  if (l < NVP) { s.qacc[l] = (l < NV) ? s.qacc_smooth[l] : 0.f; s.qfrc_con[l] = 0.f; }
  MRE_SYNC();
  if (lvalid) { s.qacc[ldof] += a; s.qfrc_con[ldof] = w; }
  if (l == 0) s.solver_iters = iters;
  MRE_SYNC();
}

MRE_PHASE_FN void solve_constraints(ModelP M, Sm& s, int l) { solve_constraints_impl<false>(M, s, l); }
MRE_PHASE_FN void solve_constraints_pyramidal(ModelP M, Sm& s, int l) { solve_constraints_impl<true>(M, s, l); }

#endif  // !MRE_NEWTON

}  // namespace mre
