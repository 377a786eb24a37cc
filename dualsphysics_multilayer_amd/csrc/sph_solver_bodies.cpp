// sph_solver_bodies.cpp — SphGpuSingle: moving boundaries, floating bodies and the step's time
// tables (sph_bodies.hip, sph_dem.hip).
#include "sph_solver_impl.hpp"

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <string>
#include <vector>

namespace sphx {

// ---- moving boundaries and floating bodies ------------------------------------------------
void SphGpuSingle::RunMotion() {
  TimedBegin(1);
  launch_motion(stream, slab() ? cap_ : npb0_, sc_, K, motion_, motmovs_, motevts_, motdata_, cur_, normal_, G);
  TimedEnd(1);
}

void SphGpuSingle::RunFloating(bool predictor) {
  TimedBegin(1);
  SLAB_TRACE("floating allreduce");
  // the body sums span the whole domain: each slab sums its owned particles, the
  // partial sums are added over the slabs, every slab integrates the same body
  launch_ft_partial(stream, sc_, ftbodies_, nftbodies_, ftridp_, arace_, cur_, ftpart_);
  if (slab() && transport_->nranks > 1) transport_->allreduce_sum_f32(ftpart_, nftbodies_ * FT_NBLK * 6, stream);
  launch_ft_body(stream, sc_, K, ftbodies_, nftbodies_, ftridp_, nftp_, cur_, predictor, ftpart_, fttab_,
                 fttabdesc_, ftnormals_ ? normal_ : nullptr);
  TimedEnd(1);
}

// The flat program: one top-level object per ref (sph_solver_set_motion).
void SphGpuSingle::SetMotion(unsigned nobj, unsigned nmov, const SphMotionMov* movs, unsigned nevt,
                             const SphMotionEvent* evts) {
  if (!nobj || nobj > unsigned(MOT_MAXOBJ)) throw SphError(SPH_ERR_UNSUPPORTED, "number of moving objects out of range");
  std::vector<SphMotionObj> nodes(nobj);
  for (unsigned k = 0; k < nobj; k++) nodes[k] = SphMotionObj{-1, int32_t(k)};
  SetMotionTree(nobj, nodes.data(), nmov, movs, nevt, evts, 0, nullptr);
}

// JDsMotion::Init (JDsMotion.cpp:94-106) + JMotion::ReadXml / ObjAdd / AxisAdd / MovAdd* /
// EventAdd / Prepare (JMotion.cpp:96-317,556-700): the program uploaded once; k_motion runs
// it every step.
void SphGpuSingle::SetMotionTree(unsigned nnode, const SphMotionObj* nodes, unsigned nmov, const SphMotionMov* movs,
                                 unsigned nevt, const SphMotionEvent* evts, unsigned nrows, const double* rows) {
  if (peri_) throw SphError(SPH_ERR_UNSUPPORTED, "moving boundaries with periodic boundaries are not implemented");
  if (inout_) throw SphError(SPH_ERR_UNSUPPORTED, "moving boundaries with inlet/outlet zones are not implemented");
  if (stepped_ || motion_) throw SphError(SPH_ERR_STATE, "the motion is configured once, before the first step");
  if (!nnode || nnode > unsigned(MOT_MAXOBJ)) throw SphError(SPH_ERR_UNSUPPORTED, "number of motion objects out of range");
  if ((nmov && !movs) || (nevt && !evts) || (nrows && !rows)) throw SphError(SPH_ERR_ARG, "motion arrays missing");
  MotionDev md;
  std::memset(&md, 0, sizeof(md));
  md.nobj = int(nnode);
  // the tree: depth first, a parent before its children, every subtree contiguous (the
  // parent of a node is the previous node or one of its ancestors)
  std::vector<int> seen(MOT_MAXOBJ, 0);
  int nref = 0;
  for (unsigned i = 0; i < nnode; i++) {
    const int p = nodes[i].parent;
    bool ok = p < 0 || (p < int(i) && p >= 0);
    if (ok && p >= 0) {
      ok = false;
      for (int q = int(i) - 1; q >= 0 && !ok; q = md.obj[q].parent) ok = (q == p);
    }
    if (!ok) throw SphError(SPH_ERR_ARG, "motion objects: not in depth-first order");
    const int r = nodes[i].ref;
    if (r >= MOT_MAXOBJ || r < -1) throw SphError(SPH_ERR_ARG, "motion objects: ref out of range");
    if (r >= 0) {
      if (seen[r]++) throw SphError(SPH_ERR_ARG, "motion objects: a ref is used twice");
      nref = std::max(nref, r + 1);
    }
    md.obj[i].parent = p;
    md.obj[i].ref = r;
  }
  for (int r = 0; r < nref; r++)  // JMotion::CreateMotList
    if (!seen[r]) throw SphError(SPH_ERR_ARG, "Motion references are no consecutives.");
  md.nref = nref;
  std::vector<MotMov> mv(std::max(nmov, 1u));
  auto find = [&](int obj, int id) -> int {
    for (unsigned k = 0; k < nmov; k++)
      if (movs[k].obj == obj && movs[k].id == id) return int(k);
    return -1;
  };
  // JMotion::AxisAdd: an axis of two distinct points is shared by the object's movements that
  // name the same points; a circular movement's reference point (p1 == p2) is its own
  auto axis_add = [&](int obj, const double* p1, const double* p2) -> int {
    const bool same = p1[0] == p2[0] && p1[1] == p2[1] && p1[2] == p2[2];
    if (!same)
      for (int k = 0; k < md.naxis; k++) {
        const MotAxis& a = md.axis[k];
        if (a.obj == obj && a.p1[0] == p1[0] && a.p1[1] == p1[1] && a.p1[2] == p1[2] && a.p2[0] == p2[0] &&
            a.p2[1] == p2[1] && a.p2[2] == p2[2])
          return k;
      }
    if (md.naxis >= MOT_MAXAXIS) throw SphError(SPH_ERR_UNSUPPORTED, "too many motion axes");
    MotAxis& a = md.axis[md.naxis];
    for (int c = 0; c < 3; c++) {
      a.p1[c] = p1[c];
      a.p2[c] = p2[c];
    }
    a.obj = obj;
    return md.naxis++;
  };
  for (unsigned k = 0; k < nmov; k++) {
    const SphMotionMov& m = movs[k];
    if (m.obj < 0 || unsigned(m.obj) >= nnode) throw SphError(SPH_ERR_ARG, "movement of an unknown object");
    if (m.type < SPH_MOV_WAIT || m.type > SPH_MOV_NULL) throw SphError(SPH_ERR_UNSUPPORTED, "movement type");
    if (m.type == SPH_MOV_WAIT && m.duration < 0)
      throw SphError(SPH_ERR_ARG, "Wating times lenght lower than zero are not allowed.");
    if (find(m.obj, m.id) != int(k)) throw SphError(SPH_ERR_ARG, "Cannot add a movement with a existing id inside the object.");
    MotMov& d = mv[k];
    std::memset(&d, 0, sizeof(d));
    d.type = m.type;
    d.prev = m.prev;
    d.fields = m.fields;
    d.time = m.duration;
    d.nextidx = -1;
    d.ax = d.rax = -1;
    if (m.next) {
      d.nextidx = find(m.obj, m.next);
      if (d.nextidx < 0) throw SphError(SPH_ERR_ARG, "movement `next` is not defined in its object");
    }
    for (int c = 0; c < 3; c++) {
      d.v[c] = m.vec[c];
      d.v2[c] = m.vec2[c];
      d.phase[c] = m.phase[c];
    }
    d.ang = m.ang;
    d.ang2 = m.ang2;
    d.ang3 = m.ang3;
    const bool rot = m.type == SPH_MOV_ROT || m.type == SPH_MOV_ROTACE || m.type == SPH_MOV_ROTSINU ||
                     m.type == SPH_MOV_ROTFILE;
    const bool cir = m.type == SPH_MOV_CIR || m.type == SPH_MOV_CIRACE || m.type == SPH_MOV_CIRSINU;
    if (rot || cir) d.ax = axis_add(m.obj, m.axisp1, m.axisp2);
    if (cir) d.rax = axis_add(m.obj, m.ref, m.ref);
    if (m.type == SPH_MOV_RECTFILE || m.type == SPH_MOV_ROTFILE) {
      if (m.data_n < 2 || size_t(m.data_first) + m.data_n > nrows)
        throw SphError(SPH_ERR_ARG, "file movement: its table rows are out of range (at least two)");
      if (m.type == SPH_MOV_RECTFILE && !(m.fields & 7)) throw SphError(SPH_ERR_ARG, "You need at least one position field.");
      d.dfirst = int(m.data_first);
      d.dn = int(m.data_n);
    }
  }
  // events ordered from last to first start, with the reference's exchange sort
  std::vector<MotEvt> ev(nevt);
  for (unsigned k = 0; k < nevt; k++) {
    if (evts[k].obj < 0 || unsigned(evts[k].obj) >= nnode) throw SphError(SPH_ERR_ARG, "event of an unknown object");
    ev[k].obj = evts[k].obj;
    ev[k].mov = find(evts[k].obj, evts[k].mov);
    if (ev[k].mov < 0) throw SphError(SPH_ERR_ARG, "event of an undefined movement");
    ev[k].start = evts[k].start;
    ev[k].finish = evts[k].finish;
  }
  for (unsigned c = 0; c + 1 < nevt; c++)
    for (unsigned c2 = c + 1; c2 < nevt; c2++)
      if (ev[c].start < ev[c2].start) std::swap(ev[c], ev[c2]);
  md.eventnext = int(nevt) - 1;
  MotionDev* dmotion = allocs_.upload(&md, 1);
  MotMov* dmovs = allocs_.upload(mv.data(), mv.size());
  MotEvt* devts = allocs_.upload(ev.data(), nevt);
  double* ddata = allocs_.upload(rows, 4 * size_t(nrows));
  motion_ = dmotion;
  motmovs_ = dmovs;
  motevts_ = devts;
  motdata_ = ddata;
  nmotobj_ = unsigned(nref);
  // restart: JDsMotion::SetTimeMod/ResetTime run the program from 0 to the PART time
  double t0 = 0;
  check_hip(hipMemcpy(&t0, &sc_->time, sizeof(double), hipMemcpyDeviceToHost), "read time");
  if (t0 > 0) launch_motion_advance(stream, sc_, motion_, motmovs_, motevts_, motdata_, 0.0, t0);
  Sync();
}

// JSph::LoadCaseConfig floating objects (JSph.cpp:1046-1100).
void SphGpuSingle::SetFloatings(unsigned nft, const SphFloatingDef* defs, double ftpause) {
  if (peri_) throw SphError(SPH_ERR_UNSUPPORTED, "floating bodies with periodic boundaries are not implemented");
  if (inout_) throw SphError(SPH_ERR_UNSUPPORTED, "floating bodies with inlet/outlet zones are not implemented");
  if (stepped_ || ftbodies_) throw SphError(SPH_ERR_STATE, "the floating bodies are configured once, before the first step");
  if (!nft || !defs) throw SphError(SPH_ERR_ARG, "no floating bodies");
  if (nn_) {
    // the v5.0 NN solver indexes its phase constants with a floating particle's code value,
    // its body index (JSphCpu_NN_FDA.cpp:199-200, 231, 267): bodies beyond the phases would
    // read past the phase table there
    if (nft > C.nphases) throw SphError(SPH_ERR_UNSUPPORTED, "NN multiphase: more floating bodies than phases");
  }
  if (C.symmetry) throw SphError(SPH_ERR_ARG, "Symmetry is not allowed with floating bodies.");  // JSph.cpp:1177
  std::vector<FtBody> b(nft);
  std::vector<float> massp(nft);
  unsigned begin = casenpb_;
  for (unsigned c = 0; c < nft; c++) {
    const SphFloatingDef& d = defs[c];
    if (d.idbegin != begin || !d.count) throw SphError(SPH_ERR_ARG, "floating blocks must follow the boundary in idp");
    FtBody& f = b[c];
    std::memset(&f, 0, sizeof(f));
    f.begin = d.idbegin - casenpb_;
    f.count = d.count;
    f.mass = float(d.massbody);
    f.massp = float(d.masspart);
    f.ftpause = float(ftpause);  // GetValueFloat (JSph.cpp:688)
    for (int k = 0; k < 9; k++) f.inertia[k] = float(d.inertia[k]);
    for (int k = 0; k < 3; k++) {
      f.center[k] = d.center[k];
      f.fvel[k] = float(d.linvelini[k]);
      f.fomega[k] = float(d.angvelini[k]);
    }
    // ComputeConstraintsValue (DualSphDef.h:456-464)
    f.constraints = (d.translationfree[0] ? 0u : 1u) | (d.translationfree[1] ? 0u : 2u) |
                    (d.translationfree[2] ? 0u : 4u) | (d.rotationfree[0] ? 0u : 8u) |
                    (d.rotationfree[1] ? 0u : 16u) | (d.rotationfree[2] ? 0u : 32u);
    massp[c] = f.massp;
    begin += d.count;
  }
  const unsigned nftp = begin - casenpb_;
  FtBody* dbodies = allocs_.upload(b.data(), nft);
  float* dmassp = allocs_.upload(massp.data(), nft);
  unsigned* dridp = allocs_.alloc<unsigned>(nftp);
  float* dpart = allocs_.alloc<float>(size_t(6) * FT_NBLK * nft);
  ftbodies_ = dbodies;
  ftmassp_ = dmassp;
  ftridp_ = dridp;
  ftpart_ = dpart;
  nftbodies_ = int(nft);
  nftp_ = nftp;
  K.nftbodies = int(nft);
  // floating p2 carry their own mass: the FT instantiation of the tiled kernel (or the
  // per-particle kernel under SPH_INTERACTION=simple / CellMode=half)
  launch_ft_ridp(stream, cap_, sc_, cur_, casenpb_, nftp_, ftridp_, K, G);
  Sync();
}

// RigidAlgorithm (JSph.cpp:599-603): FTMODE_Ext's pair rule in the interaction kernels and, with
// use_dem, the StDemData table of the DEM pass (JSph.cpp:1114-1130) and DemDtForce (JSph.cpp:
// 2091-2098: DtIni, or the restart PART's value).
void SphGpuSingle::SetRigid(int ftmode, bool use_dem, unsigned ndem, const SphDemDef* dem, double demdtforce) {
  if (ftmode != SPH_FTMODE_SPH && ftmode != SPH_FTMODE_EXT) throw SphError(SPH_ERR_ARG, "Rigid algorithm is not valid.");
  if (ftmode == SPH_FTMODE_SPH) {
    if (use_dem) throw SphError(SPH_ERR_ARG, "DEM needs SPH_FTMODE_EXT (RigidAlgorithm=2)");
    if (ftext_) throw SphError(SPH_ERR_STATE, "the rigid algorithm is configured once, before the first step");
    return;
  }
  if (slab()) throw SphError(SPH_ERR_ARG, "RigidAlgorithm 0 and 2 (FTMODE_Ext, DEM) run on a single domain only");
  if (stepped_ || ftext_) throw SphError(SPH_ERR_STATE, "the rigid algorithm is configured once, before the first step");
  if (!ftbodies_) throw SphError(SPH_ERR_STATE, "configure the floating bodies before their rigid algorithm");
  const char* bad = nn_ ? "NN multiphase" : normal_ ? "mDBC" : ext_ ? (sps_ ? "Laminar+SPS viscosity" : "Shifting") : nullptr;
  if (bad) throw SphError(SPH_ERR_UNSUPPORTED, std::string(bad) + " with RigidAlgorithm 0 or 2 is not implemented");
  if (use_dem) {
    if (!ndem || !dem) throw SphError(SPH_ERR_ARG, "DEM needs the data of every boundary block");
    std::vector<DemRec> tab(DEM_TABLE);
    std::memset(tab.data(), 0, sizeof(DemRec) * tab.size());
    std::vector<char> have(DEM_TABLE, 0);
    for (unsigned i = 0; i < ndem; i++) {
      const SphDemDef& d = dem[i];
      if (d.code >= DEM_TABLE || d.code >= unsigned(CODE_TYPE_FLUID)) throw SphError(SPH_ERR_ARG, "DEM data: not a boundary block's code");
      if (have[d.code]) throw SphError(SPH_ERR_ARG, "DEM data: a block is given twice");
      have[d.code] = 1;
      DemRec& r = tab[d.code];
      r.mass = d.mass;
      r.tau = d.tau;
      r.kfric = d.kfric;
      r.restitu = d.restitu;
      r.massp = d.massp;
    }
    for (int c = 0; c < nftbodies_; c++)
      if (!have[unsigned(CODE_TYPE_FLOATING) + unsigned(c)]) throw SphError(SPH_ERR_ARG, "DEM data: a floating body has none");
    check_hip(hipSetDevice(device), "hipSetDevice");
    DemRec* dtab = allocs_.upload(tab.data(), tab.size());
    const double d0 = demdtforce > 0 ? demdtforce : C.dtini;
    Sync();
    check_hip(hipMemcpy(&sc_->demdtforce, &d0, sizeof(double), hipMemcpyHostToDevice), "set DemDtForce");
    demtab_ = dtab;
  }
  ftext_ = true;
}

// FtLinearVel / FtAngularVel / FtLinearForce / FtAngularForce of one body (JSph.cpp:1060-1082):
// the rows are re-uploaded as one buffer with a {first row, rows} descriptor per table.
void SphGpuSingle::SetFloatingTable(unsigned body, int kind, unsigned n, const double* times, const double* values) {
  if (stepped_) throw SphError(SPH_ERR_STATE, "floating tables are configured before the first step");
  if (!ftbodies_ || body >= unsigned(nftbodies_)) throw SphError(SPH_ERR_ARG, "floating table of an unknown body");
  if (kind < SPH_FTTAB_LINVEL || kind > SPH_FTTAB_ANGFORCE) throw SphError(SPH_ERR_ARG, "invalid floating table kind");
  // External forces: v5.2 adds them to FtoForces before FtCalcForces adds the particle sums
  // (sum + (0 + ext)); the v5.0 NN solver adds them inside FtCalcForces after the sums
  // (FtSumExternalForces, JSphCpuSingle.cpp:849 of that solver): the same float additions, so
  // both run k_ft_forces's (sph_bodies.hip).
  if (!n || !times || !values) throw SphError(SPH_ERR_ARG, "There are not times.");
  std::vector<double4> rows(n);
  for (unsigned i = 0; i < n; i++) {  // rows in the order given (any time order, as the reference)
    const double* v = values + 3 * size_t(i);
    if (kind >= SPH_FTTAB_LINFORCE && (v[0] == DBL_MAX || v[1] == DBL_MAX || v[2] == DBL_MAX))
      throw SphError(SPH_ERR_ARG, "external forces have no 'none' components");
    rows[i] = make_double4(times[i], v[0], v[1], v[2]);
  }
  fttabs_.resize(size_t(nftbodies_) * 4);
  fttabs_[size_t(body) * 4 + size_t(kind)] = rows;
  UploadFloatingTables();
}

void SphGpuSingle::UploadFloatingTables() {
  if (fttabs_.empty()) return;
  std::vector<double4> all;
  std::vector<FtTabDesc> desc(fttabs_.size());
  for (size_t t = 0; t < fttabs_.size(); t++) {
    desc[t] = FtTabDesc{int(all.size()), int(fttabs_[t].size()), -1, -1, 0.0};
    all.insert(all.end(), fttabs_[t].begin(), fttabs_[t].end());
  }
  Sync();
  // the new tables first, then the old ones go: a failure leaves the solver with the old ones
  double4* dtab = allocs_.upload(all.data(), all.size());
  FtTabDesc* ddesc = allocs_.upload(desc.data(), desc.size());
  std::swap(fttab_, dtab);
  std::swap(fttabdesc_, ddesc);
  allocs_.release(dtab);
  allocs_.release(ddesc);
}

// DtFixedFile (JDsFixedDt) and ViscoTime (JDsViscoInput) tables on the device; k_dt reads
// them at every DtVariable (fixed dt) and at every step's end (the next step's Visco).
void SphGpuSingle::SetTimeTable(int kind, unsigned n, const double* times, const double* values) {
  if (kind != SPH_TTAB_DTFIXED && kind != SPH_TTAB_VISCO) throw SphError(SPH_ERR_ARG, "invalid time table kind");
  if (n == 1 || (n && (!times || !values))) throw SphError(SPH_ERR_ARG, "Cannot be less than two values.");
  if (kind == SPH_TTAB_DTFIXED && n && C.dtfixed > 0)
    throw SphError(SPH_ERR_ARG, "The parameters 'DtFixed' and 'DtFixedFile' cannot be used at the same time.");
  // NN multiphase: ViscoTime sets Visco every step (JSphCpuSingle.cpp:1128 of the v5.0 solver),
  // which no NN interaction reads (they take the phases' viscosities, JSphCpu_NN_FDA.cpp:267,
  // JSphCpu_NN_SPH.cpp:202,413): the table is kept and, as there, changes nothing.
  Sync();
  // the new table first (times [n], then values [n]), then the old one goes
  void* fresh = nullptr;
  if (n && kind == SPH_TTAB_DTFIXED) {
    std::vector<double> h(times, times + n);
    h.insert(h.end(), values, values + n);
    fresh = allocs_.upload(h.data(), h.size());
  } else if (n) {  // JDsViscoInput reads float rows (ReadNextFloat)
    std::vector<float> h(2 * size_t(n));
    for (unsigned i = 0; i < n; i++) {
      h[i] = float(times[i]);
      h[n + i] = float(values[i]);
    }
    fresh = allocs_.upload(h.data(), h.size());
  }
  check_hip(hipMemset(kind == SPH_TTAB_DTFIXED ? &sc_->dtfix_pos : &sc_->visco_pos, 0, sizeof(int)), "reset table row");
  void*& buf = (kind == SPH_TTAB_DTFIXED ? dttab_ : viscotab_);
  std::swap(buf, fresh);
  allocs_.release(fresh);
  if (kind == SPH_TTAB_DTFIXED) {
    K.dtfix_n = int(n);
    K.dtfix_t = (const double*)buf;
    K.dtfix_v = n ? K.dtfix_t + n : nullptr;
  } else {
    K.visco_n = int(n);
    K.visco_t = (const float*)buf;
    K.visco_v = n ? K.visco_t + n : nullptr;
    launch_visco_init(stream, sc_, K);
    Sync();
  }
}

unsigned SphGpuSingle::Floatings(SphFloatingState* out, unsigned cap) {
  if (!nftbodies_) return 0;
  std::vector<FtBody> b(nftbodies_);
  Sync();
  check_hip(hipMemcpy(b.data(), ftbodies_, sizeof(FtBody) * b.size(), hipMemcpyDeviceToHost), "read floatings");
  for (unsigned c = 0; c < unsigned(nftbodies_) && c < cap && out; c++) {
    SphFloatingState& o = out[c];
    std::memset(&o, 0, sizeof(o));
    for (int k = 0; k < 3; k++) {
      o.center[k] = b[c].center[k];
      o.fvel[k] = b[c].fvel[k];
      o.fomega[k] = b[c].fomega[k];
      o.angles[k] = b[c].angles[k];
      o.facelin[k] = b[c].facelin[k];
      o.faceang[k] = b[c].faceang[k];
    }
  }
  return unsigned(nftbodies_);
}

}  // namespace sphx
