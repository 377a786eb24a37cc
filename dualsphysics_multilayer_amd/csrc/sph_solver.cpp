// sph_solver.cpp — host orchestration (see sph_solver.hpp): construction, memory, the phases of a
// step, results.
#include "sph_solver_impl.hpp"
#include "sph_items.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace sphx {

// Test hooks read from the environment (buffer sizing, item cutting, slab turns) change how a
// run is executed, never its results; a production run must not pick one up silently, so the
// first one met is reported once on stderr.
void test_hook_notice(const char* name) {
  static bool said = false;
  if (said) return;
  said = true;
  std::fprintf(stderr, "libsphcore: test hook %s is set in the environment (measurement / test mode)\n", name);
}

void check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) throw SphError(SPH_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

SphGpuSingle::SphGpuSingle(const SphCaseDef& cdef, const SphParticlesHost& init, int dev) : device(dev) {
  Init(cdef, init);
}

SphGpuSingle::SphGpuSingle(const SphCaseDef& cdef, const SphParticlesHost& all, int dev, const SlabConfig& slab,
                           std::unique_ptr<SlabTransport> transport)
    : device(dev), transport_(std::move(transport)), slabcfg_(slab) {
  if (!transport_) throw SphError(SPH_ERR_ARG, "slab without a transport");
  if (transport_->rank != slab.rank || transport_->nranks != slab.nranks)
    throw SphError(SPH_ERR_ARG, "slab rank does not match the transport");
  Init(cdef, all);
}

void SphGpuSingle::Init(const SphCaseDef& cdef, const SphParticlesHost& init) {
  derive_constants(cdef, C);
  K = make_kconst(C);
  G = make_grid(C, slab() ? &slabcfg_ : nullptr);
  step_algorithm_ = cdef.step_algorithm;
  if (init.n != cdef.np) throw SphError(SPH_ERR_ARG, "particle count does not match the case");
  if (!init.n) throw SphError(SPH_ERR_ARG, "no particles");
  // Particles this solver holds: all (single domain) or owned + ghost columns (slab).
  std::vector<unsigned> sel;
  unsigned nown = init.n;
  if (slab()) {
    const std::vector<unsigned> cx = initial_columns(C, init, slabcfg_.axis);
    const int W = ghost_width(C);
    const int lo = slabcfg_.c0 - (slabcfg_.rank > 0 ? W : 0);
    const int hi = slabcfg_.c1 + (slabcfg_.rank + 1 < slabcfg_.nranks ? W : 0);
    nown = 0;
    for (unsigned p = 0; p < init.n; p++) {
      const int c = int(cx[p]);
      if (c >= lo && c < hi) sel.push_back(p);
      if (c >= slabcfg_.c0 && c < slabcfg_.c1) nown++;
    }
    if (sel.empty()) throw SphError(SPH_ERR_ARG, "slab without particles");
  } else {
    sel.resize(init.n);
    for (unsigned p = 0; p < init.n; p++) sel[p] = p;
  }
  npb0_ = 0;
  for (unsigned p : sel) npb0_ += (p < cdef.npb ? 1u : 0u);
  casenpb_ = cdef.npb;
  const unsigned n = unsigned(sel.size());
  if (const char* e = std::getenv("SPH_SLAB_MINCAP")) slab_mincap_ = slab() && std::atoi(e) != 0;
  if (const char* e = std::getenv("SPH_SLAB_CUT")) cut_items_ = slab() && std::atoi(e) != 0;
  if (slab_mincap_ || cut_items_) test_hook_notice(slab_mincap_ ? "SPH_SLAB_MINCAP" : "SPH_SLAB_CUT");
  cap_ = slab() ? n + (slab_mincap_ ? 16u : std::max(n / 2, 65536u)) : n;
  // Periodic boundaries: single domain, DBC, one phase, artificial viscosity, no bodies (the
  // set_* calls refuse those).  The duplicates live behind the normal particles, and at a
  // divide the new ones are appended while the previous divide's still hold their slots (the
  // sort drops those): the capacity is the normal particles + twice the first divide's
  // duplicates + head-room (half as many again, at least 4096), sized once; a divide that
  // needs more stops the run (ERR_PERI_FULL).
  peri_ = C.peri_active != 0;
  if (peri_) {
    if (slab()) throw SphError(SPH_ERR_UNSUPPORTED, "periodic boundaries are not implemented for slab solvers");
    if (C.tboundary == SPH_BOUND_MDBC) throw SphError(SPH_ERR_UNSUPPORTED, "periodic boundaries with mDBC are not implemented");
    if (C.rheology == SPH_RHEOLOGY_NN)
      throw SphError(SPH_ERR_UNSUPPORTED, "periodic boundaries with NN multiphase are not implemented");
    if (C.tvisco != SPH_VISCO_ARTIFICIAL || C.shift_mode != SPH_SHIFT_NONE)
      throw SphError(SPH_ERR_UNSUPPORTED, "periodic boundaries with Laminar+SPS or shifting are not implemented");
    if (C.symmetry) throw SphError(SPH_ERR_UNSUPPORTED, "periodic boundaries with Symmetry are not implemented");
    if (init.code)
      for (unsigned p = 0; p < init.n; p++) {
        const typecode t = CodeType(init.code[p]);
        if (t == CODE_TYPE_MOVING || t == CODE_TYPE_FLOATING)
          throw SphError(SPH_ERR_UNSUPPORTED,
                         "periodic boundaries with moving boundaries or floating bodies are not implemented");
      }
    P_ = make_periconst(C);
    const unsigned ndup = initial_periodic_count(C, init, cdef.npb);
    if (const char* e = std::getenv("SPH_PERI_MINCAP")) peri_mincap_ = std::atoi(e) != 0;
    if (peri_mincap_) test_hook_notice("SPH_PERI_MINCAP");
    const unsigned long long want = 0ull + n + 2ull * ndup + (peri_mincap_ ? 0u : std::max(ndup / 2, 4096u));
    if (want >= (1ull << 31)) throw SphError(SPH_ERR_ARG, "The number of particles is too big.");
    cap_ = unsigned(want);
  }
  keybits_ = bits_for(G.boxdiscard, 1);
  // grid-sized buffers hold the widest grid a slab can get from a re-partition (all cells
  // of the slab axis + W = ghost_width ghost cells per face), so they never move
  gmax_ncx_ = int(C.dom_cells[0]) + (slab() && slabcfg_.axis == 0 ? 2 * ghost_width(C) : 0);
  gmax_ncy_ = int(C.dom_cells[1]) + (slab() && slabcfg_.axis == 1 ? 2 * ghost_width(C) : 0);
  nctmax_ = slab() ? unsigned(gmax_ncx_) * unsigned(gmax_ncy_) * unsigned(G.ncz) : G.nct;
  if (slab() && slabcfg_.axis == 1) {
    if (C.dom_cells[1] < 2u) throw SphError(SPH_ERR_UNSUPPORTED, "y-slabs of a 2-D case (one y row)");
    if (C.symmetry) throw SphError(SPH_ERR_UNSUPPORTED, "Symmetry (the y = 0 mirror) on y-slabs");
  }
  if (const char* e = std::getenv("SPH_INTERACTION")) tiled_ = std::string(e) != "simple";
  if (const char* e = std::getenv("SPH_COMM_TIMEOUT_S")) comm_timeout_s_ = std::max(1.0, std::atof(e));
  // incremental divide: distinct key offsets of the 27 neighbour cells (ncx >= 3, checked
  // again per divide for a re-partitioned slab; ncy >= 3 or a single y row), 30-bit counts
  inc_ok_ = G.ncx >= 3 && (G.ncy >= 3 || G.ncy == 1) && n < (1u << 29);
  if (const char* e = std::getenv("SPH_DIVIDE")) inc_ok_ = inc_ok_ && std::string(e) != "full";
  // periodic cases take the full sort every divide, as the reference does with PeriActive
  // (JCellDivCpuSingle.cpp:298): the duplicates are appended behind np and re-sorted
  if (peri_) inc_ok_ = false;
  if (const char* e = std::getenv("SPH_CLS_SPLIT")) cls_split_ = std::atoi(e) != 0;
  if (cls_split_) test_hook_notice("SPH_CLS_SPLIT");
  // The tiled kernel stages the 3x3 rows of 3 cells of CellMode=full, or the 5x5 rows of
  // 5 half-cells of CellMode=half (run_pass_half).
  nn_ = (C.rheology == SPH_RHEOLOGY_NN);
  nnsph_ = nn_ && C.velgrad == SPH_VELGRAD_SPH;
  casenp_ = cdef.np;
  shift_ = (C.shift_mode != SPH_SHIFT_NONE);
  sps_ = !nn_ && C.tvisco == SPH_VISCO_LAMINARSPS;
  ext_ = !nn_ && (sps_ || shift_);
  facex_ = slab() && (nnsph_ || sps_);
  mdbc_corrector_ = cdef.tboundary == SPH_BOUND_MDBC && cdef.mdbc_corrector != 0;
  if (ext_) tiled_ = true;
  if (C.kernel == SPH_KERNEL_CUBIC && nn_)
    throw SphError(SPH_ERR_UNSUPPORTED, "the Cubic spline kernel with NN multiphase is not implemented");
  if (C.kernel == SPH_KERNEL_CUBIC && !tiled_)
    throw SphError(SPH_ERR_UNSUPPORTED, "the Cubic spline kernel runs on the tiled interaction only");
  if (C.symmetry && !tiled_) throw SphError(SPH_ERR_UNSUPPORTED, "Symmetry runs on the tiled interaction only");
  if (slab()) {
    // the first interaction's face records (NN / SPS / mDBC face re-sends): the initial
    // particles of the face and ghost columns (both sides of a face count the same
    // particles); later from each exchange
    const std::vector<unsigned> cx = initial_columns(C, init, slabcfg_.axis);
    const bool hl = slabcfg_.rank > 0, hr = slabcfg_.rank + 1 < slabcfg_.nranks;
    const int W = ghost_width(C), c0 = slabcfg_.c0, c1 = slabcfg_.c1;
    for (unsigned p : sel) {
      const int c = int(cx[p]);
      face_sl_ += (hl && c >= c0 && c < c0 + W) ? 1u : 0u;
      face_sr_ += (hr && c >= c1 - W && c < c1) ? 1u : 0u;
      face_rl_ += (hl && c >= c0 - W && c < c0) ? 1u : 0u;
      face_rr_ += (hr && c >= c1 && c < c1 + W) ? 1u : 0u;
    }
  }
  if (nn_) {
    // the NN interaction is the tiled kernel of sph_nn.hip only (full or half cells)
    tiled_ = true;
  }
  check_hip(hipSetDevice(device), "hipSetDevice");
  check_hip(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
  try {
    AllocFixed();
    if (nn_) UploadPhases(cdef);
    AllocParticles(cap_);
    if (slab()) PresizeExchange(init);
    Upload(init, sel, nown);
    if (C.tboundary == SPH_BOUND_MDBC) UploadNormals(cdef, init);
    // ConfigDomain: RunCellDivide(true) (JSphCpuSingle.cpp:165-166), then InitRunGpu.
    RunCellDivide();
    exchange_armed_ = true;
    if (step_algorithm_ == SPH_STEP_VERLET)
      check_hip(hipMemcpyAsync(cur_.velrhopm1, cur_.velrhop, sizeof(float4) * cap_, hipMemcpyDeviceToDevice, stream),
                "init VelrhopM1");
    Sync();
    CheckErrors();
  } catch (...) {
    Free();
    (void)hipStreamDestroy(stream);
    stream = nullptr;
    throw;
  }
}

SphGpuSingle::~SphGpuSingle() {
  if (xstream_) (void)hipStreamSynchronize(xstream_);
  if (stream) (void)hipStreamSynchronize(stream);
  Free();
  for (auto& e : pending_) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto e : evpool_) (void)hipEventDestroy(e);
  if (xev_) (void)hipEventDestroy(xev_);
  if (ev_div_) (void)hipEventDestroy(ev_div_);
  if (ev_ghost_) (void)hipEventDestroy(ev_ghost_);
  if (xstream_) {
    (void)hipStreamSynchronize(xstream_);
    (void)hipStreamDestroy(xstream_);
  }
  if (stream) (void)hipStreamDestroy(stream);
}

void SphGpuSingle::AllocFixed() {
  begincell_ = allocs_.alloc<unsigned>(2 * size_t(nctmax_) + 6);
  if (slab()) {  // re-partition: column counts [2 ncx] + the ranks' bounds [nranks + 1]
    colcnt_ = allocs_.alloc<float>(2 * size_t(C.dom_cells[slabcfg_.axis]) + size_t(slabcfg_.nranks) + 1);
  }
  // two lists x (fluid, bound) rows of item counts, for the widest grid of the run
  rowtmp_ = allocs_.alloc<unsigned>(ITEMS_ROWTMP(std::max(G.ncy, gmax_ncy_), G.ncz));
  // the count pass's staged items (sph_items.hpp), sized for the widest grid of the run
  ricap_ = ITEMS_RICAP(std::max(G.ncx, gmax_ncx_));
  // test hook: smaller slots send more rows down the place pass's second walk
  // (tests/test_gpu_items.py checks the run is bitwise the same)
  if (const char* e = std::getenv("SPH_ITEMS_RICAP")) ricap_ = std::max(1u, std::min(ricap_, unsigned(std::atoi(e))));
  rowitems_ = allocs_.alloc<uint4>((ITEMS_ROWTMP(std::max(G.ncy, gmax_ncy_), G.ncz) - 1) * ricap_);
  qctr_ = allocs_.alloc<unsigned>(QCTR_BYTES / sizeof(unsigned));
  check_hip(hipMemset(qctr_, 0, QCTR_BYTES), "zero work counters");
  sort_.digtot = allocs_.alloc<unsigned>(1u << RS_MAXBITS);
  if (inc_ok_) {
    begincell_alt_ = allocs_.alloc<unsigned>(2 * size_t(nctmax_) + 6);
    inc_.stayoff = allocs_.alloc<unsigned>(2 * size_t(nctmax_) + 6);
    inc_.nb2 = inc_blocks_boxes(G.nctt);
    if (const char* e = std::getenv("SPH_INC_DBG")) inc_.dbg = std::atoi(e);
    inc_.ctr = allocs_.alloc<unsigned>(QSTRIDE);
    check_hip(hipMemset(inc_.ctr, 0, 4 * QSTRIDE), "zero far count");
  }
  if (facex_) idxmap_ = allocs_.alloc<unsigned>(size_t(std::max(casenp_, 1u)));
  sc_ = allocs_.alloc<DevScalars>(1);
  dttrace_ = allocs_.alloc<double>(size_t(tracecap_));
  pairs_ = allocs_.alloc<unsigned long long>(6);
  folded_ = allocs_.alloc<unsigned>(8);
  slabcnt_ = allocs_.alloc<SlabCounts>(1);
  // the accumulated counts (nkeep, ghosts) start at zero; k_unpack_finish zeroes them again
  // at the end of every exchange
  check_hip(hipMemset(slabcnt_, 0, sizeof(SlabCounts)), "zero slab counts");
  if (slab()) {
    // face messages and their prefixes (the ghost exchange after the divide); the second
    // item list and its counters
    faces_.W = ghost_width(C);
    faces_.nfb = 2u * face_boxes_per_type(G, faces_.W);  // the full extent of the other axes: fixed
    for (int k = 0; k < 4; k++) {
      // the send messages' face-box counts accumulate in k_pack_count from zero; k_face_scan
      // zeroes them again once it has their prefixes
      faces_.msg[k] = allocs_.alloc<unsigned>(size_t(FMSG_HDR) + faces_.nfb);
      check_hip(hipMemset(faces_.msg[k], 0, 4 * (size_t(FMSG_HDR) + faces_.nfb)), "zero face messages");
      faces_.pre[k] = allocs_.alloc<unsigned>(size_t(faces_.nfb) + 1);
    }
    qctrf_ = allocs_.alloc<unsigned>(QCTR_BYTES / sizeof(unsigned));
    check_hip(hipMemset(qctrf_, 0, QCTR_BYTES), "zero work counters");
  }
  check_hip(hipHostMalloc((void**)&sc_host_, sizeof(DevScalars), hipHostMallocDefault), "hipHostMalloc");
  check_hip(hipHostMalloc((void**)&slabcnt_host_, sizeof(SlabCounts), hipHostMallocDefault), "hipHostMalloc");
}

// NN phase tables (JSph::InitMultiPhase + ConfigConstantsMP): the interaction's constants
// (sph_device.hpp layout) and the EOS of every phase for the divide's pressure.
void SphGpuSingle::UploadPhases(const SphCaseDef& cdef) {
  // rows [0, 2 NN_MAXPH): {mass, cs0, visco, tau_yield}, {m, n, tau_max, bi_multi} per phase;
  // rows [2 NN_MAXPH, 3 NN_MAXPH): per-phase products of the pair bodies, in float as the
  // kernels formed them per pair: {m tau_yield, -m log2(e), n - 1, DDTkh cs0}
  std::vector<float4> tab(3 * NN_MAXPH, make_float4(0.f, 0.f, 0.f, 0.f)), eos(NN_MAXPH, make_float4(1.f, 0.f, 1.f, 0.f));
  for (unsigned p = 0; p < C.nphases; p++) {
    const SphPhaseDef& ph = cdef.phases[p];
    tab[2 * p] = make_float4(C.phase_mass[p], float(ph.cs0), float(ph.visco), float(ph.tau_yield));
    tab[2 * p + 1] = make_float4(float(ph.hbp_m), float(ph.hbp_n), float(ph.tau_max), float(ph.bi_multi));
    if (float(ph.tau_max) != 0.f) K.nnbi = 1;  // the pair bodies take the bi-viscosity branch
    const float m = float(ph.hbp_m);
    tab[2 * NN_MAXPH + p] = make_float4(m * float(ph.tau_yield), -m * 1.4426950408889634f, float(ph.hbp_n) - 1.f,
                                        K.ddtkh * float(ph.cs0));
    const float gam = float(ph.gamma) ? float(ph.gamma) : C.gamma;
    const int ig = (gam == float(int(gam)) && gam >= 1.f && gam <= 16.f) ? int(gam) : 0;
    eos[p] = make_float4(float(ph.rho), C.phase_cteb[p], gam, float(ig));
    phase_rho_[p] = float(ph.rho);
  }
  phasek_ = allocs_.upload(tab.data(), tab.size());
  phaseeos_ = allocs_.alloc<float4>(3 * NN_MAXPH);
  check_hip(hipMemcpy(phaseeos_, eos.data(), sizeof(float4) * eos.size(), hipMemcpyHostToDevice), "upload phases");
}

// Everything sized by the particle capacity (both gather sets, sort scratch, slab tiles).
void SphGpuSingle::AllocParticles(unsigned cap) {
  const size_t n = cap;
  for (PartArrays* a : {&cur_, &alt_}) {
    *a = PartArrays();
    a->idp = pallocs_.alloc<unsigned>(n);
    a->code = pallocs_.alloc<typecode>(n);
    a->dcell = pallocs_.alloc<unsigned>(n);
    a->posxy = pallocs_.alloc<double2>(n);
    a->posz = pallocs_.alloc<double>(n);
    a->velrhop = pallocs_.alloc<float4>(n);
    if (sps_) a->tau = pallocs_.alloc<float4>(2 * n);
    if (step_algorithm_ == SPH_STEP_VERLET) {
      a->velrhopm1 = pallocs_.alloc<float4>(n);
    } else {
      a->posxypre = pallocs_.alloc<double2>(n);
      a->poszpre = pallocs_.alloc<double>(n);
      a->velrhoppre = pallocs_.alloc<float4>(n);
    }
  }
  poscell_ = pallocs_.alloc<float4>(n);
  press_ = pallocs_.alloc<float>(n);
  // Interaction items (launch_items): an item holds TB particles unless it ends a row
  // (<= 2 per row: fluid and bound) or reaches TMAXCELLS = 4 cells (<= 1 per 4 cells).
  // (slabs: up to three column ranges per row)
  items_ = pallocs_.alloc<uint4>(n / 128 + 6 * size_t(G.ncy) * size_t(G.ncz) + size_t(nctmax_) / 2 + 2);
  arace_ = pallocs_.alloc<float4>(n);
  if (shift_) shiftpos_ = pallocs_.alloc<float4>(n);  // the interaction's shifting sums
  if (sps_) taunew_ = pallocs_.alloc<float4>(2 * n);
  if (nnsph_) {
    viscoeta_ = pallocs_.alloc<float>(n);
    if (C.tvisco == SPH_VISCO_CONSTEQ) tau_ = pallocs_.alloc<float4>(2 * n);
  }
  for (int i = 0; i < 2; i++) {
    sort_.keys[i] = pallocs_.alloc<unsigned>(n);
    sort_.vals[i] = pallocs_.alloc<unsigned>(n);
  }
  if (inc_ok_) {
    inc_.nb1 = inc_blocks_classify(n);
    const size_t ns = size_t(inc_.nb1) * INC_TILE_SIZE;  // tile-major mover slots
    inc_.skeys = pallocs_.alloc<unsigned>(n);
    inc_.newkey = pallocs_.alloc<unsigned>(n);
    inc_.cw = pallocs_.alloc<unsigned>(n);
    inc_.fidx = pallocs_.alloc<unsigned>(n);
    inc_.mkey = pallocs_.alloc<unsigned>(ns);
    inc_.mposnear = pallocs_.alloc<unsigned>(ns);
    inc_.mfar = pallocs_.alloc<uint2>(n);
    inc_.mposfar = pallocs_.alloc<unsigned>(n);
    inc_.tagg = pallocs_.alloc<uint2>(size_t(inc_.nb1));
    inc_.tpg = pallocs_.alloc<unsigned>(size_t(inc_.nb1));
    const size_t nsup = (size_t(inc_.nb1) + 63) / 64;
    inc_.tsup = pallocs_.alloc<unsigned long long>(TSUP_STRIDE * nsup);
    check_hip(hipMemset(inc_.tsup, 0, 8 * TSUP_STRIDE * nsup), "zero super tiles");
    inc_valid_ = false;  // new scratch: the next divide is a full one
  }
  if (slab()) {
    // new positions of the appended particles and reserved ghost slots (either divide)
    inc_.apppos = pallocs_.alloc<unsigned>(n);
  }
  sort_.ntiles = unsigned((n + RS_TILE - 1) / RS_TILE);
  sort_.hist = pallocs_.alloc<unsigned>(size_t(sort_.ntiles) * (1u << RS_MAXBITS));
  // slab pack tile counts: tilecnt[7][ntiles] (ghost L/R, migrant L/R, staying, face ghosts L/R; sph_slab.hip)
  packtiles_ = pallocs_.alloc<unsigned>(PK_TILECNT_BYTES(n) / sizeof(unsigned));
  if (peri_) periscan_ = pallocs_.alloc<unsigned>(peri_scan_words(cap));
  if (inout_) {
    ioscan_ = pallocs_.alloc<unsigned>(inout_scan_words(cap));
    ionewiz_ = pallocs_.alloc<unsigned char>(n);
    iolist_ = pallocs_.alloc<unsigned>(n);
  }
  cap_ = cap;
}

void SphGpuSingle::FreeParticles() {
  pallocs_.clear();
}

// The device arenas and the growing buffers free themselves with the solver (their members'
// destructors, also after a constructor that threw); the arenas go here, before the streams.
void SphGpuSingle::Free() {
  FreeParticles();
  allocs_.clear();
  if (sc_host_) (void)hipHostFree(sc_host_);
  if (slabcnt_host_) (void)hipHostFree(slabcnt_host_);
  sc_host_ = nullptr;
  slabcnt_host_ = nullptr;
}

// Slab capacity growth (a slab gains particles as the fluid moves across it): new
// arrays, the live [0, np_live) of the current set copied over, the old set freed.
// (A failure in here ends the solver's use: the old set goes with `oldallocs`, once, and
// what was allocated of the new one with the solver.)
void SphGpuSingle::Grow(unsigned np_live, unsigned newcap) {
  check_hip(hipStreamSynchronize(stream), "grow: sync");
  const PartArrays old = cur_;
  DevArena oldallocs;
  oldallocs.swap(pallocs_);
  AllocParticles(newcap);
  auto cp = [&](void* dst, const void* src, size_t bytes) {
    if (src && dst && bytes) check_hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream), "grow: copy");
  };
  const size_t n = np_live;
  cp(cur_.idp, old.idp, 4 * n);
  cp(cur_.code, old.code, 2 * n);
  cp(cur_.dcell, old.dcell, 4 * n);
  cp(cur_.posxy, old.posxy, 16 * n);
  cp(cur_.posz, old.posz, 8 * n);
  cp(cur_.velrhop, old.velrhop, 16 * n);
  cp(cur_.velrhopm1, old.velrhopm1, 16 * n);
  cp(cur_.posxypre, old.posxypre, 16 * n);
  cp(cur_.poszpre, old.poszpre, 8 * n);
  cp(cur_.velrhoppre, old.velrhoppre, 16 * n);
  cp(cur_.tau, old.tau, 32 * n);
  check_hip(hipStreamSynchronize(stream), "grow: copy");
  oldallocs.clear();
}

void SphGpuSingle::Upload(const SphParticlesHost& h, const std::vector<unsigned>& sel, unsigned nown) {
  const unsigned n = unsigned(sel.size());
  std::vector<unsigned> dcell(n), idp(n);
  std::vector<typecode> code(n);
  std::vector<double2> pxy(n);
  std::vector<double> pz(n);
  std::vector<float4> vr(n);
  for (unsigned i = 0; i < n; i++) {
    const unsigned p = sel[i];
    idp[i] = h.idp[p];
    const double x = h.pos[3 * p], y = h.pos[3 * p + 1], z = h.pos[3 * p + 2];
    pxy[i] = make_double2(x, y);
    pz[i] = z;
    vr[i] = make_float4(h.vel[3 * p], h.vel[3 * p + 1], h.vel[3 * p + 2], h.rhop[p]);
    // LoadCodeParticles (JSph.cpp:1257): the codes of the case's MK blocks when given,
    // else one fixed and one fluid block.
    if (h.code) {
      code[i] = h.code[p];
      const typecode t = CodeType(code[i]);
      if (!CodeIsNormal(code[i]) || (i < npb0_) != (t < CODE_TYPE_FLOATING))
        throw SphError(SPH_ERR_ARG, "particle codes: boundary (fixed/moving) particles must be the first npb");
    } else {
      code[i] = (i < npb0_ ? typecode(0) : CODE_TYPE_FLUID);
    }
    // JSph::LoadMultiphaseData (JSph.cpp:3248-3263 of the v5.0 solver): a fluid particle's
    // density starts at its phase's rho; its code value must name a phase.
    if (nn_ && CodeIsFluid(code[i])) {
      const unsigned ph = code[i] & CODE_MASKVALUE;
      if (ph >= C.nphases) throw SphError(SPH_ERR_ARG, "Fluid particle without phase information...");
      vr[i].w = phase_rho_[ph];
    }
    // JSph::CheckRhopLimits (JSph.cpp:2021-2030).
    if (i >= npb0_ && (vr[i].w < C.rhopoutmin || C.rhopoutmax < vr[i].w))
      throw SphError(SPH_ERR_ARG, "Initial fluid density is out of limits.");
    // JSph::LoadDcellParticles (JSph.cpp:1690-1711).
    const double dx = x - C.dom_posmin[0], dy = y - C.dom_posmin[1], dz = z - C.dom_posmin[2];
    {  // inside the real map (without periodic axes DomPosMin is MapRealPosMin: the same values)
      const double rx = peri_ ? x - C.map_realposmin[0] : dx, ry = peri_ ? y - C.map_realposmin[1] : dy,
                   rz = peri_ ? z - C.map_realposmin[2] : dz;
      if (!(rx >= 0 && ry >= 0 && rz >= 0 && rx < C.map_realsize[0] && ry < C.map_realsize[1] && rz < C.map_realsize[2]))
        throw SphError(SPH_ERR_ARG, "Found new particles out.");
    }
    dcell[i] = DcelCell(C.dom_cellcode, unsigned(dx / double(C.scell)), unsigned(dy / double(C.scell)),
                        unsigned(dz / double(C.scell)));
  }
  check_hip(hipMemcpy(cur_.idp, idp.data(), 4 * size_t(n), hipMemcpyHostToDevice), "upload idp");
  check_hip(hipMemcpy(cur_.code, code.data(), 2 * size_t(n), hipMemcpyHostToDevice), "upload code");
  check_hip(hipMemcpy(cur_.dcell, dcell.data(), 4 * size_t(n), hipMemcpyHostToDevice), "upload dcell");
  check_hip(hipMemcpy(cur_.posxy, pxy.data(), 16 * size_t(n), hipMemcpyHostToDevice), "upload posxy");
  check_hip(hipMemcpy(cur_.posz, pz.data(), 8 * size_t(n), hipMemcpyHostToDevice), "upload posz");
  check_hip(hipMemcpy(cur_.velrhop, vr.data(), 16 * size_t(n), hipMemcpyHostToDevice), "upload velrhop");
  // InitRunCpu: SpsTauc = 0 (JSphCpu.cpp:423)
  if (cur_.tau) check_hip(hipMemset(cur_.tau, 0, 32 * size_t(cap_)), "zero tau");
  DevScalars s;
  std::memset(&s, 0, sizeof(s));
  s.np = n;
  s.npb = npb0_;
  s.npbok = npb0_;
  s.nown = nown;
  s.symdtpre = C.dtini;  // InitRun (JSph.cpp:2090)
  check_hip(hipMemcpy(sc_, &s, sizeof(s), hipMemcpyHostToDevice), "upload scalars");
  verletstep_ = 0;
}

// JSph::LoadBoundNormals + ConfigBoundNormals (JSph.cpp:1265-1340): the case's normals
// (particle -> boundary limit) as float, doubled (particle -> ghost node), kept by idp.
void SphGpuSingle::UploadNormals(const SphCaseDef& cdef, const SphParticlesHost& h) {
  if (!h.boundnormal) throw SphError(SPH_ERR_ARG, "mDBC needs the boundary normals (<case>_Normals.nbi4)");
  // normals by idp: the boundary's [0, CaseNpb) and, when the floating bodies have normals
  // (UseNormalsFt, JSph.cpp:1301-1306: mDBC on them too), theirs up to the last one given
  unsigned nnor = cdef.npb, nftnor = 0;
  for (unsigned p = 0; p < h.n; p++) {
    const unsigned id = h.idp[p];
    if (id < cdef.npb) continue;
    const float x = h.boundnormal[3 * p], y = h.boundnormal[3 * p + 1], z = h.boundnormal[3 * p + 2];
    if (x != 0.f || y != 0.f || z != 0.f) {
      nnor = std::max(nnor, id + 1);
      nftnor++;
    }
  }
  ftnormals_ = nftnor > 0;
  nnormal_ = nnor;
  std::vector<float4> nor(std::max(nnor, 1u), make_float4(0.f, 0.f, 0.f, 0.f));
  unsigned nerr = 0;
  for (unsigned p = 0; p < h.n; p++) {
    const unsigned id = h.idp[p];
    if (id >= nnor) continue;
    const float x = h.boundnormal[3 * p], y = h.boundnormal[3 * p + 1], z = h.boundnormal[3 * p + 2];
    if (id < cdef.npb && x == 0.f && y == 0.f && z == 0.f) nerr++;
    nor[id] = make_float4(x * 2.f, y * 2.f, z * 2.f, 0.f);
  }
  if (nerr == cdef.npb && !ftnormals_) throw SphError(SPH_ERR_ARG, "No valid normal vectors for using mDBC.");
  normal_ = allocs_.upload(nor.data(), nor.size());
  if (slab()) {
    // face-column boundary (and floating) records: sized per interaction from the exchange's
    // face sizes (MdbcFaceExchange); the idp -> index map of those particles
    bidx_ = allocs_.alloc<unsigned>(std::max(nnor, 1u));
  }
  // boundary particles migrate between slabs, but a slab never holds more boundary
  // particles (owned + ghost) than the case has: CaseNpb bounds every slab's npbok, so
  // the list and sums keep their size when Grow() raises the particle capacity (and the
  // floating particles with normals bound the floating part of the list)
  const size_t nlist = size_t(slab() ? cdef.npb : npb0_) + nftnor + 1;
  mdbclist_ = allocs_.alloc<unsigned>(nlist);
  mdbcsums_ = allocs_.alloc<char>(MDBC_SUM_BYTES * nlist);
}

// Restart: TimeStep and SymplecticDtPre of the loaded PART (JSph::InitRun, JSph.cpp:2094-2106).
void SphGpuSingle::SetTime(double time, double symdtpre) {
  if (inout_)  // JSphCpuSingle_InOut.cpp:76
    throw SphError(SPH_ERR_UNSUPPORTED, "Simulation restart not allowed when Inlet/Outlet is used.");
  if (motion_) throw SphError(SPH_ERR_STATE, "set the restart time before the motion (it is advanced to that time)");
  UploadFloatingTables();  // the floating tables' lookups start over (a restart's new JLinearValues)
  Sync();
  check_hip(hipMemcpy(&sc_->time, &time, sizeof(double), hipMemcpyHostToDevice), "set time");
  // the tables' walks start again from their first rows (a restarted reference run loads them anew)
  check_hip(hipMemset(&sc_->dtfix_pos, 0, 2 * sizeof(int)), "reset table rows");
  if (accstate_) check_hip(hipMemset(accstate_, 0xff, sizeof(AccState) * ACC_MAXIN), "reset acceleration tables");
  if (symdtpre > 0)
    check_hip(hipMemcpy(&sc_->symdtpre, &symdtpre, sizeof(double), hipMemcpyHostToDevice), "set SymplecticDtPre");
  if (K.visco_n) {  // ViscoTime at the restart time
    launch_visco_init(stream, sc_, K);
    Sync();
  }
}

// ---- timing -----------------------------------------------------------------------
void SphGpuSingle::SetTiming(bool on) {
  Sync();
  timing_ = on;
  for (int i = 0; i < 4; i++) { phase_ms_[i] = 0; phase_n_[i] = 0; }
}
// Phases timed (bit i: phase i of phase_ms_; all by default).  Every event pair is a marker
// in the stream, so a run timing only the interaction keeps the other launches back to back.
void SphGpuSingle::SetTimingPhases(unsigned mask) {
  Sync();
  timing_mask_ = mask & 0xfu;
}
void SphGpuSingle::TimedBegin(int phase) {
  if (!timing_ || !((timing_mask_ >> phase) & 1u)) return;
  hipEvent_t a;
  if (!evpool_.empty()) { a = evpool_.back(); evpool_.pop_back(); }
  else check_hip(hipEventCreate(&a), "hipEventCreate");
  check_hip(hipEventRecord(a, stream), "hipEventRecord");
  cur_a_ = a;
}
void SphGpuSingle::TimedEnd(int phase) {
  if (!timing_ || !((timing_mask_ >> phase) & 1u)) return;
  hipEvent_t b;
  if (!evpool_.empty()) { b = evpool_.back(); evpool_.pop_back(); }
  else check_hip(hipEventCreate(&b), "hipEventCreate");
  check_hip(hipEventRecord(b, stream), "hipEventRecord");
  pending_.push_back(Ev{cur_a_, b, phase});
}
void SphGpuSingle::Timing(double out_ms[4], uint64_t* launches) {
  Sync();
  for (auto& e : pending_) {
    float ms = 0;
    check_hip(hipEventElapsedTime(&ms, e.a, e.b), "hipEventElapsedTime");
    phase_ms_[e.phase] += ms;
    phase_n_[e.phase]++;
    evpool_.push_back(e.a);
    evpool_.push_back(e.b);
  }
  pending_.clear();
  for (int i = 0; i < 4; i++) out_ms[i] = phase_n_[i] ? phase_ms_[i] / double(phase_n_[i]) : 0.0;
  if (launches) *launches = phase_n_[0];
}

// ---- phases ------------------------------------------------------------------------

void SphGpuSingle::RunCellDivide() {
  // turns measurement mode: the divide's kernels after the exchange are a turn of their own
  // and the timed divide phase is those kernels alone (the exchange waits for neighbours)
  const bool turn = slab() && exchange_armed_ && in_run_ && transport_->turns();
  if (!turn) TimedBegin(2);
  // the update's classification was made for this divide (FuseUpdate's prediction): a phase
  // order that breaks it must not merge with stale classes
  if (classified_ && fuse_pre_ != havepre_)
    throw SphError(SPH_ERR_STATE, "internal: the update classified the particles for another divide");
  if (slab() && exchange_armed_ && repart_every_ && (stepsdone_ % repart_every_) == 0 && transport_->nranks > 1 &&
      !havepre_)
    Repartition();
  // the exchange of this divide: ghosts in reserved slots, their records after the sort
  const bool ghosts = slab() && exchange_armed_ && (transport_->has_left() || transport_->has_right());
  if (slab() && exchange_armed_) Exchange();
  if (turn) {
    transport_->turn_wait(SlabTransport::TURN_DIVIDE, stream, nullptr);
    TimedBegin(2);
  }
  const unsigned ngl = ghosts ? unsigned(xg_rl_) : 0u, ngr = ghosts ? unsigned(xg_rr_) : 0u;
  const bool withm1 = (step_algorithm_ == SPH_STEP_VERLET);
  // RunPeriodic before every divide, the in-step one of Symplectic included (JSphCpuSingle.cpp:444)
  if (peri_) launch_run_periodic(stream, cap_, sc_, P_, K, cur_, withm1, havepre_, periscan_);
  // InOutComputeStep at the end-of-step divide (JSphCpuSingle_InOut.cpp:146-210): the zones' rules
  // and the new inlet particles behind np
  if (inout_ && io_pass_ == 2) launch_inout_step(stream, cap_, sc_, iodev_, K, cur_, ioscan_, ionewiz_);
  // Items (each build also zeroes its queues).  With the overlap a slab cuts its rows where
  // the stencil (scelldiv columns) stops reaching a ghost column: the interior list runs
  // while the ghost records are in flight, the face list (items of <= scelldiv columns) after
  // them.  With the ghosts in place the rows are not cut (full items); SPH_SLAB_CUT=1 cuts
  // them there too, which makes the two modes bitwise the same (a test hook).
  const bool overlap = ghosts && OverlapGhosts();
  ghost_split_ = false;
  ItemBuild ib;
  if (tiled_) {
    const int S = int(C.scelldiv), hl = slab() && transport_->has_left(), hr = slab() && transport_->has_right();
    // the owned cells along the slab axis whose stencil (scelldiv cells) reaches no ghost
    int ib0 = G.sown0 + (hl ? S : 0), ie0 = G.sown1 - (hr ? S : 0);
    if (ib0 >= ie0) ib0 = ie0 = G.sown0;  // a narrow slab: every item reaches a ghost cell
    const bool inc = inc_ok_ && inc_valid_ && G.ncx >= 3 && (G.ncy >= 3 || G.ncy == 1);
    const unsigned* bcnew = inc ? begincell_alt_ : begincell_;  // the begincell this divide writes
    if (overlap) {  // the interior list (qctr_), then the face list (qctrf_) after it
      const int xr[6] = {ib0, ie0, G.sown0, ib0, ie0, G.sown1};
      ib = make_item_build(bcnew, G, rowtmp_, items_, qctr_, C.scelldiv, xr, qctrf_, rowitems_, ricap_);
      ghost_split_ = true;
    } else if (cut_items_) {  // the overlap's items in one list (SPH_SLAB_CUT test hook)
      const int xa[6] = {G.sown0, ib0, ib0, ie0, ie0, G.sown1};
      ib = make_item_build(bcnew, G, rowtmp_, items_, qctr_, C.scelldiv, xa, nullptr, rowitems_, ricap_);
    } else {
      // ghosts in place: the rows' items over all owned columns, as in one domain (a row cut
      // at the face columns leaves items of one cell there, ~1/3 of the block's lanes)
      ib = make_item_build(bcnew, G, rowtmp_, items_, qctr_, C.scelldiv, nullptr, nullptr, rowitems_, ricap_);
    }
  }
  if (inc_ok_ && inc_valid_ && G.ncx >= 3 && (G.ncy >= 3 || G.ncy == 1)) {
    // the previous order merged with the particles whose box changed and, on a slab, the
    // particles the exchange appended and the ghosts' slots (sph_divide.hip); the item
    // count runs in the push launch, the item write right after it
    inc_.nb2 = inc_blocks_boxes(G.nctt);
    launch_divide_inc(stream, cap_, sc_, cur_, alt_, withm1, havepre_, K, C.dom_posmin, poscell_, press_, G, begincell_,
                      begincell_alt_, inc_, sort_, keybits_, nn_ ? phaseeos_ : nullptr, ghosts ? &faces_ : nullptr, ngl,
                      ngr, tiled_ ? &ib : nullptr, classified_);
    std::swap(begincell_, begincell_alt_);
  } else {
    // the ghosts' slots sort as entries [np, np + ngl + ngr) after the particles
    launch_presort(stream, cap_, sc_, cur_.dcell, cur_.code, G, C.dom_cellcode, sort_.keys[0], sort_.vals[0], ngl + ngr);
    if (ngl + ngr)
      launch_ghost_keys(stream, faces_, G, ngl, ngr, sort_.keys[0] + xg_np_, sort_.vals[0] + xg_np_, xg_np_);
    const int res = launch_radix_sort(stream, cap_, sc_, sort_, keybits_);
    launch_begincell(stream, cap_, sc_, sort_.keys[res], G, begincell_);
    launch_gather(stream, cap_, sc_, sort_.vals[res], cur_, alt_, withm1, havepre_, K, C.dom_posmin, poscell_, press_,
                  G.offx(), G.offy(), nn_ ? phaseeos_ : nullptr, ghosts ? xg_np_ : ~0u, xg_np_ - xg_nm_, inc_.apppos);
    if (inc_ok_)
      check_hip(hipMemcpyAsync(inc_.skeys, sort_.keys[res], 4 * size_t(cap_), hipMemcpyDeviceToDevice, stream),
                "keep sorted keys");
    if (tiled_) launch_items(stream, ib);
  }
  inc_valid_ = inc_ok_;
  classified_ = false;
  inc_.napp = 0;
  inc_.nvl = inc_.nvr = 0;
  std::swap(cur_, alt_);
  qpass_ = 0;
  if (ghosts) {
    // this slab's ghost records for the neighbours, from its sorted face columns, posted at
    // once.  With the overlap they are packed on the exchange stream, so the interaction's
    // interior items follow the divide directly on the solver stream; the transfer and the
    // scatter follow in the interaction (also, in the turns measurement mode, the in-place
    // transfer: it is then part of the slab's own interaction turn).
    hipStream_t gs = stream;
    if (overlap) {
      ExchangeStream();
      check_hip(hipEventRecord(ev_div_, stream), "divide: event");
      check_hip(hipStreamWaitEvent(xstream_, ev_div_, 0), "ghosts: wait divide");
      gs = xstream_;
    }
    launch_ghost_pack(gs, sc_, faces_, G, begincell_, cur_, poscell_, send_, unsigned(xg_sl_), unsigned(xg_sr_));
    transport_->post(send_.gl, sizeof(SlabGhost) * xg_sl_, send_.gr, sizeof(SlabGhost) * xg_sr_, gs);
    if (overlap || (transport_->turns() && OverlapEligible())) {
      ghost_pending_ = true;
    } else {
      GhostCollect(stream);
    }
  }
  if (nftp_) launch_ft_ridp(stream, cap_, sc_, cur_, casenpb_, nftp_, ftridp_, K, G);
  // InOutUpdatePartsData after it (JSphCpuSingle_InOut.cpp:216-217, 228-255)
  if (inout_ && io_pass_)
    launch_inout_parts(stream, cap_, sc_, iodev_, ioh_, K, G, cur_, begincell_, press_, iolist_, withm1);
  TimedEnd(2);
  if (turn) transport_->turn_done(SlabTransport::TURN_DIVIDE, stream);
}

unsigned SphGpuSingle::NextQueueCopy() {
  const unsigned c = qpass_ % QCTR_COPIES;
  if (++qpass_ > unsigned(QCTR_COPIES)) {  // beyond the copies the item build zeroed
    check_hip(hipMemsetAsync(qctr_ + c * QCTR_WORDS, 0, QCTR_QUEUE_BYTES, stream), "zero work counters");
    if (ghost_split_)
      check_hip(hipMemsetAsync(qctrf_ + c * QCTR_WORDS, 0, QCTR_QUEUE_BYTES, stream), "zero work counters");
  }
  return c * QCTR_WORDS;
}

void SphGpuSingle::Interaction_Forces(int interstep) {
  bool t0 = false;  // the interaction's timed interval has begun
  auto begin0 = [&] {
    if (!t0) TimedBegin(0);
    t0 = true;
  };
  // turns measurement mode (SPH_SLAB_TURNS, in-process slabs): this slab's interaction starts
  // on the GPU after the previous slab's has ended
  const bool turn = slab() && transport_->turns();
  if (turn) {
    ExchangeStream();
    transport_->turn_wait(SlabTransport::TURN_INTERACTION, stream, xstream_);
  }
  if (ghost_pending_ && !ghost_split_) {  // deferred in-place ghosts: the transfer is timed with it
    begin0();
    GhostCollect(stream);
    ghost_pending_ = false;
  }
  // mDBC boundary correction first, except in the Symplectic corrector unless MDBCCorrector
  // (JSphCpuSingle.cpp:525); with floating normals the floating particles too (JSphCpu.cpp:1199).
  if (normal_ && (mdbc_corrector_ || interstep != 3)) {
    TimedBegin(3);
    launch_mdbc(stream, slab() ? cap_ : npb0_, sc_, cur_, press_, normal_, begincell_, G, K, C.dom_posmin, C.mdbc_threshold,
                mdbclist_ + 1, mdbclist_, mdbcsums_, ftnormals_ ? ftridp_ : nullptr, ftnormals_ ? nftp_ : 0u);
    if (slab() && (transport_->has_left() || transport_->has_right())) MdbcFaceExchange();
    TimedEnd(3);
  }
  const unsigned qc = tiled_ ? NextQueueCopy() : 0u;
  unsigned *qa = qctr_ + qc, *qf = qctrf_ ? qctrf_ + qc : nullptr;
  if (nn_) {
    // NN multiphase (sph_nn.hip); the shifting sums only where they are applied: the
    // corrector (the predictor's RunShifting result is never used, shift=false in
    // ComputeSymplecticPre) and Verlet
    begin0();
    launch_nn_tiled(stream, nblocks_tiled_, sc_, items_, qa, poscell_, cur_.velrhop, press_, cur_.code, begincell_,
                    G, K, phasek_, arace_, shiftpos_, shift_ && interstep != 2, viscoeta_, tau_, ftmassp_);
    if (nnsph_) {
      // SPH velocity gradients: the viscous force is a second pass over the neighbours,
      // reading their effective viscosities / stress tensors (JSphCpu_NN_SPH.cpp:671-696)
      if (slab() && C.tvisco != SPH_VISCO_ARTIFICIAL && (transport_->has_left() || transport_->has_right()))
        NNFaceExchange();
      launch_nn_visc(stream, nblocks_tiled_, sc_, items_, qctr_ + NextQueueCopy(), poscell_, cur_.velrhop, cur_.code, viscoeta_, tau_,
                     begincell_, G, K, phasek_, arace_, ftmassp_);
    }
  } else if (ext_) {
    // Laminar+SPS and/or shifting (sph_ext.hip).  Slabs with SPS: the ghosts' tau (the
    // owners' from the last interaction) first
    if (sps_ && slab() && (transport_->has_left() || transport_->has_right())) NNFaceExchange();
    begin0();
    launch_fluid_ext(stream, nblocks_tiled_, sc_, items_, qa, poscell_, cur_.velrhop, press_, cur_.code, ftmassp_,
                     cur_.tau, begincell_, G, K, arace_, shiftpos_, taunew_, interstep != 2);
    if (sps_) std::swap(cur_.tau, taunew_);
  } else if (tiled_) {
    // The tiled kernel writes the arace of every owned particle (skipped boundary items
    // get ar = 0); its work queues are the copy NextQueueCopy picked.
    begin0();  // the timed interval is the interaction kernel alone (rocprof's per-kernel average)
    if (ghost_pending_) {
      // Slab: the interior items now, the ghost records in flight on the exchange stream
      // (packed and posted there after the divide); there the face items follow their
      // arrival.  The interior kernel leaves a few block slots free so that the transfer and
      // scatter kernels start at once.
      launch_fluid_tiled(stream, nblocks_tiled_, sc_, items_, qa, poscell_, cur_.velrhop, press_, begincell_, G, K,
                         arace_, cur_.code, ftmassp_, 64, ftext_);
      GhostCollect(xstream_);
      launch_fluid_tiled(xstream_, nblocks_tiled_, sc_, items_, qf, poscell_, cur_.velrhop, press_, begincell_, G,
                         K, arace_, cur_.code, ftmassp_, 0, ftext_);
      check_hip(hipEventRecord(ev_ghost_, xstream_), "ghosts: event");
      check_hip(hipStreamWaitEvent(stream, ev_ghost_, 0), "ghosts: join");
      ghost_pending_ = false;
    } else {
      launch_fluid_tiled(stream, nblocks_tiled_, sc_, items_, qa, poscell_, cur_.velrhop, press_, begincell_, G, K,
                         arace_, cur_.code, ftmassp_, 0, ftext_);
      if (ghost_split_)  // the ghosts are in: the face items right after
        launch_fluid_tiled(stream, nblocks_tiled_, sc_, items_, qf, poscell_, cur_.velrhop, press_, begincell_,
                           G, K, arace_, cur_.code, ftmassp_, 0, ftext_);
    }
  } else {
    begin0();
    launch_interaction(stream, cap_, sc_, poscell_, cur_.velrhop, press_, begincell_, G, K, arace_, cur_.code,
                       ftmassp_, ftext_);
  }
  if (demtab_) {
    // JSphCpu::InteractionForcesDEM (JSphCpu.cpp:975), added onto the pair sums; its dt goes
    // into the ViscDt slots.  AceMax starts over: a contact can lower the |ace| that held the
    // pair-sum maximum, and k_dem reduces the final |ace|^2 of [npb, np).
    check_hip(hipMemsetAsync(&sc_->red[RED_ACEMAX2][0], 0, 4 * RED_SLOTS, stream), "reset acemax");
    launch_dem(stream, cap_, sc_, K, G, float(C.dp), demtab_, begincell_, cur_, interstep, arace_);
  }
  if (acc_.n) {
    // JDsAccInput::RunCpu (JSphCpu.cpp:444), added onto the pair sums.  The interaction's
    // AceMax is of the pair sums alone and no bound of the total: its slots start over and
    // k_accinput reduces the final |ace|^2 of [npb, np).
    check_hip(hipMemsetAsync(&sc_->red[RED_ACEMAX2][0], 0, 4 * RED_SLOTS, stream), "reset acemax");
    launch_accinput(stream, cap_, sc_, K, G, acc_, accrows_, accstate_, accvals_, interstep, cur_, arace_);
  }
  if (peri_) {
    // AceMax over the normal particles only (ComputeAceMax, JSphCpuSingle.cpp:584-605): a
    // duplicate in the rim beyond the real map lacks the neighbours further out
    check_hip(hipMemsetAsync(&sc_->red[RED_ACEMAX2][0], 0, 4 * RED_SLOTS, stream), "reset acemax");
    launch_peri_acemax(stream, cap_, sc_, cur_.code, arace_);
  }
  if (inout_) {
    // AceMax over the normal particles that are not inout (ComputeAceMax, JSphCpuSingle.cpp:584-605)
    check_hip(hipMemsetAsync(&sc_->red[RED_ACEMAX2][0], 0, 4 * RED_SLOTS, stream), "reset acemax");
    launch_inout_acemax(stream, cap_, sc_, cur_.code, arace_);
  }
  TimedEnd(0);
  if (turn && fold_turn_ >= 0) {  // the next DtVariable's fold, inside this slab's turn
    launch_fold_maxima(stream, sc_, folded_, fold_turn_ != 0);
    folded_ready_ = true;
  }
  fold_turn_ = -1;
  if (turn) transport_->turn_done(SlabTransport::TURN_INTERACTION, stream);
}

void SphGpuSingle::DtVariable(int mode) {
  if (slab() && transport_->nranks > 1) {  // one rank: its own maxima are the domain's
    SLAB_TRACE("dt allreduce");
    // The three maxima span the whole domain: fold locally, max over all slabs.
    if (!folded_ready_) launch_fold_maxima(stream, sc_, folded_, mode != DT_PEEK);
    folded_ready_ = false;
    transport_->allreduce_max_u32(folded_, 5, stream);  // 4 maxima + the fatal error flags
    launch_dt(stream, sc_, K, C.cflnumber, C.dtmin, C.cs0, mode, dttrace_, tracecap_, folded_);
  } else {
    launch_dt(stream, sc_, K, C.cflnumber, C.dtmin, C.cs0, mode, dttrace_, tracecap_);
  }
}

// Turns measurement mode 2 (SPH_SLAB_TURNS=2, in-process slabs): the update kernels are a
// turn of their own.
void SphGpuSingle::UpdateTurn(bool begin) {
  if (!(slab() && in_run_ && transport_->turns())) return;
  if (begin) transport_->turn_wait(SlabTransport::TURN_UPDATE, stream, nullptr);
  else transport_->turn_done(SlabTransport::TURN_UPDATE, stream);
}

// The next divide's classification (sph_incdiv.hpp) and, on a slab with neighbours, its
// exchange's count pass (sph_slabpack.hpp) in the update kernel: the next divide is
// incremental and nothing moves a particle between the update and the divide (no floating
// bodies, no moving boundaries; no re-partition at that divide, which changes the slab's
// columns and hence every key).  pre_at_divide: whether the Symplectic pre-state is held at
// the divide (the re-partition's condition; RunCellDivide checks that it holds what was
// predicted here).  SPH_CLS_SPLIT=1 (test hook, read at construction) keeps the separate
// k_inc_classify and k_pack_count launches.
SphGpuSingle::UpdateFuse SphGpuSingle::FuseUpdate(bool pre_at_divide) {
  classified_ = packcounted_ = false;
  UpdateFuse f;
  const bool repart = slab() && exchange_armed_ && repart_every_ && (stepsdone_ % repart_every_) == 0 &&
                      transport_->nranks > 1 && !pre_at_divide;
  if (cls_split_ || repart || !inc_ok_ || !inc_valid_ || !(G.ncx >= 3 && (G.ncy >= 3 || G.ncy == 1)) || nftbodies_ ||
      nmotobj_ || inc_.napp != 0)
    return f;
  classified_ = true;
  fuse_pre_ = pre_at_divide;
  fused_updates_++;
  f.cls = &inc_;
  const bool hl = slab() && transport_->has_left(), hr = slab() && transport_->has_right();
  if (slab() && exchange_armed_ && (hl || hr)) {
    pack_args_ = make_pack_args(cap_, cur_, G, K, C.dom_posmin, hl, hr, step_algorithm_ == SPH_STEP_VERLET,
                                pre_at_divide, packtiles_, slabcnt_, send_, normal_, nnormal_, &faces_);
    packcounted_ = true;
    f.pk = &pack_args_;
  }
  return f;
}

void SphGpuSingle::ComputeVerlet() {
  UpdateTurn(true);
  TimedBegin(1);
  verletstep_++;
  const bool euler = !(verletstep_ < C.verlet_steps);
  const UpdateFuse fu = FuseUpdate(false);
  if (inout_) launch_update_inout(stream, cap_, sc_, K, 0, euler, arace_, cur_, G);
  else
    launch_verlet(stream, cap_, sc_, K, euler, arace_, cur_, G, shift_ ? shiftpos_ : nullptr, fu.cls, fu.pk,
                  peri_ ? &P_ : nullptr);
  if (euler) verletstep_ = 0;
  std::swap(cur_.velrhop, cur_.velrhopm1);
  TimedEnd(1);
  UpdateTurn(false);
}

void SphGpuSingle::ComputeSymplecticPre() {
  UpdateTurn(true);
  TimedBegin(1);
  std::swap(cur_.posxy, cur_.posxypre);
  std::swap(cur_.posz, cur_.poszpre);
  std::swap(cur_.velrhop, cur_.velrhoppre);
  havepre_ = true;
  const UpdateFuse fu = FuseUpdate(true);
  if (inout_) launch_update_inout(stream, cap_, sc_, K, 1, false, arace_, cur_, G);
  else launch_sym_pre(stream, cap_, sc_, K, arace_, cur_, G, fu.cls, fu.pk, peri_ ? &P_ : nullptr);
  TimedEnd(1);
  UpdateTurn(false);
}

void SphGpuSingle::ComputeSymplecticCorr() {
  UpdateTurn(true);
  TimedBegin(1);
  const UpdateFuse fu = FuseUpdate(false);
  if (inout_) launch_update_inout(stream, cap_, sc_, K, 2, false, arace_, cur_, G);
  else
    launch_sym_cor(stream, cap_, sc_, K, arace_, cur_, G, shift_ ? shiftpos_ : nullptr, fu.cls, fu.pk,
                   peri_ ? &P_ : nullptr);
  havepre_ = false;
  TimedEnd(1);
  UpdateTurn(false);
}

void SphGpuSingle::ComputeStep() {
  stepped_ = true;
  stepsdone_++;
  // (turns mode: each interaction's turn ends with the fold of the DtVariable after it)
  const bool foldturn = slab() && transport_->nranks > 1 && transport_->turns();
  if (step_algorithm_ == SPH_STEP_VERLET) {
    if (foldturn) fold_turn_ = 1;
    Interaction_Forces(1);
    DtVariable(DT_VERLET);
    ComputeVerlet();
    if (nftbodies_) RunFloating(false);
  } else {
    if (foldturn) fold_turn_ = 1;
    Interaction_Forces(2);
    DtVariable(DT_SYM_PRE);
    ComputeSymplecticPre();
    if (nftbodies_) RunFloating(true);
    RunCellDivide();
    if (foldturn) fold_turn_ = 1;
    Interaction_Forces(3);
    DtVariable(DT_SYM_COR);
    ComputeSymplecticCorr();
    if (nftbodies_) RunFloating(false);
  }
  if (ndamp_) RunDamping();  // after the last update and RunFloating (JSphCpuSingle.cpp:683,717)
  if (gauges_.ng) RunGauges();  // at TimeStep + stepdt, before the motion and the divide (JSphCpuSingle.cpp:1095)
  if (nmotobj_) RunMotion();
  io_pass_ = inout_ ? 2 : 0;  // InOutComputeStep in place of the plain divide (JSphCpuSingle.cpp:1097)
  RunCellDivide();
  io_pass_ = 0;
}

void SphGpuSingle::PhaseDt(bool final_) {
  check_hip(hipSetDevice(device), "hipSetDevice");
  if (step_algorithm_ == SPH_STEP_VERLET) DtVariable(final_ ? DT_VERLET : DT_PEEK);
  else DtVariable(final_ ? DT_SYM_COR : DT_SYM_PRE);
}

void SphGpuSingle::PhaseUpdate(int interstep) {
  if (nmotobj_ || nftbodies_)
    throw SphError(SPH_ERR_UNSUPPORTED,
                   "the update phases do not move a motion program's boundaries or floating bodies: step such a "
                   "solver with sph_solver_run");
  if ((interstep == 1) != (step_algorithm_ == SPH_STEP_VERLET))
    throw SphError(SPH_ERR_STATE, "the update phase is not one of the solver's step algorithm");
  check_hip(hipSetDevice(device), "hipSetDevice");
  // ComputeStep's bookkeeping, once per step: stepsdone_ is read by this update's FuseUpdate
  // and by the divides after it (a slab's re-partition schedule), as inside ComputeStep
  stepped_ = true;
  if (interstep != 3) stepsdone_++;
  if (interstep == 1) ComputeVerlet();
  else if (interstep == 2) ComputeSymplecticPre();
  else ComputeSymplecticCorr();
  if (ndamp_ && interstep != 2) RunDamping();  // as ComputeStep: not after the predictor
}

void SphGpuSingle::Run(unsigned nsteps) {
  check_hip(hipSetDevice(device), "hipSetDevice");
  in_run_ = true;
  try {
    for (unsigned s = 0; s < nsteps; s++) ComputeStep();
    GhostFinish();  // the state between runs is whole (ghosts in place)
  } catch (...) {
    in_run_ = false;
    throw;
  }
  in_run_ = false;
  check_hip(hipGetLastError(), "kernel launch");
}

void SphGpuSingle::Sync() { check_hip(hipStreamSynchronize(stream), "hipStreamSynchronize"); }

SphRunStats SphGpuSingle::Stats() {
  check_hip(hipMemcpyAsync(sc_host_, sc_, sizeof(DevScalars), hipMemcpyDeviceToHost, stream), "read scalars");
  Sync();
  const DevScalars& s = *sc_host_;
  SphRunStats r;
  std::memset(&r, 0, sizeof(r));
  r.time = s.time;
  r.last_dt = s.last_dt;
  r.sym_dtpre = s.symdtpre;
  r.nstep = s.nstep;
  // a slab reports the particles it owns (no ghosts); alone it holds exactly those
  r.np = (slab() && (transport_->has_left() || transport_->has_right())) ? s.nown : s.np;
  r.npb = s.npb;
  r.npbok = s.npbok;
  if (peri_) {  // normal particles only: the duplicates sit among them in the cells
    r.npbper = s.npbper;
    r.npfper = s.npfper;
    r.np = s.np - s.npbper - s.npfper;
    r.npb = s.npb - s.npbper;
    r.npbok = s.npbok - std::min(s.npbok, s.npbper);
  }
  r.nout = s.nout;
  r.dtmodif = s.dtmodif;
  r.error_flags = s.error_flags;
  r.velmax = s.last_velmax;
  r.acemax = s.last_acemax;
  r.viscdtmax = s.last_viscdt;
  r.viscetadtmax = s.last_visceta;
  r.fused_updates = fused_updates_;
  r.dem_dtforce = demtab_ ? s.demdtforce : 0.0;
  return r;
}

void SphGpuSingle::CheckErrors() {
  const SphRunStats s = Stats();
  if (s.error_flags & ERR_BOUNDOUT) throw SphError(SPH_ERR_BOUNDOUT, "boundary particles were excluded (AbortBoundOut)");
  if (s.error_flags & ERR_DT_NAN) throw SphError(SPH_ERR_DT, "The computed Dt is NaN or infinity");
  if (s.error_flags & ERR_PERI_FULL)
    throw SphError(SPH_ERR_NOMEM, "the periodic duplicates of a divide exceed the particle capacity (step " +
                                      std::to_string(s.nstep) + ")");
  if (s.error_flags & ERR_INOUT_FULL)
    throw SphError(SPH_ERR_NOMEM, "the new inlet particles of a step exceed the particle capacity (step " +
                                      std::to_string(s.nstep) + ")");
  if (s.error_flags & ERR_HALO_NODE)
    throw SphError(SPH_ERR_UNSUPPORTED, "slab halo: an mDBC ghost node needs particles beyond the slab's ghost columns");
  if (s.error_flags & ERR_HALO_FACE)
    throw SphError(SPH_ERR_STATE, "slab halo: a face record did not fit its buffer (step " + std::to_string(s.nstep) +
                                      ", " + HaloDiag() + ")");
  if (s.error_flags & ERR_HALO_MISS)
    throw SphError(SPH_ERR_STATE, "slab halo: a face record found no ghost copy of its particle");
  if (s.error_flags & ERR_HALO_GHOST)
    throw SphError(SPH_ERR_STATE, "slab halo: a ghost record the divide did not place (face counts disagree)");
}

unsigned SphGpuSingle::DtTrace(double* out, unsigned cap) {
  const SphRunStats s = Stats();
  const unsigned n = unsigned(std::min<unsigned long long>(s.nstep, tracecap_));
  if (out && cap) {
    std::vector<double> all(tracecap_);
    check_hip(hipMemcpy(all.data(), dttrace_, 8 * size_t(tracecap_), hipMemcpyDeviceToHost), "read dt trace");
    const unsigned long long first = s.nstep - n;
    for (unsigned i = 0; i < n && i < cap; i++) out[i] = all[(first + i) % tracecap_];
  }
  return n;
}

void SphGpuSingle::Download(SphParticlesHost& out) {
  const SphRunStats s = Stats();
  const unsigned n = sc_host_->np;  // held particles (a slab also holds ghosts)
  if (out.n < s.np) throw SphError(SPH_ERR_ARG, "output buffer too small");
  std::vector<double2> pxy(n);
  std::vector<double> pz(n);
  std::vector<float4> vr(n);
  std::vector<unsigned> idp(n), dcell(n);
  std::vector<typecode> code(n);
  check_hip(hipMemcpy(pxy.data(), cur_.posxy, 16 * size_t(n), hipMemcpyDeviceToHost), "download posxy");
  check_hip(hipMemcpy(pz.data(), cur_.posz, 8 * size_t(n), hipMemcpyDeviceToHost), "download posz");
  check_hip(hipMemcpy(vr.data(), cur_.velrhop, 16 * size_t(n), hipMemcpyDeviceToHost), "download velrhop");
  check_hip(hipMemcpy(idp.data(), cur_.idp, 4 * size_t(n), hipMemcpyDeviceToHost), "download idp");
  check_hip(hipMemcpy(code.data(), cur_.code, 2 * size_t(n), hipMemcpyDeviceToHost), "download code");
  if (slab()) check_hip(hipMemcpy(dcell.data(), cur_.dcell, 4 * size_t(n), hipMemcpyDeviceToHost), "download dcell");
  unsigned k = 0;
  for (unsigned p = 0; p < n; p++) {
    if (slab()) {  // owned particles only
      if (!slab_owned(G, slab_local(G, C.dom_cellcode, dcell[p]))) continue;
    }
    if (peri_ && !CodeIsNormal(code[p])) continue;  // normal particles only (GetParticlesData onlynormal)
    if (k >= out.n) throw SphError(SPH_ERR_STATE, "owned particle count mismatch");
    if (out.idp) out.idp[k] = idp[p];
    if (out.code) out.code[k] = code[p];
    if (out.pos) { out.pos[3 * k] = pxy[p].x; out.pos[3 * k + 1] = pxy[p].y; out.pos[3 * k + 2] = pz[p]; }
    if (out.vel) { out.vel[3 * k] = vr[p].x; out.vel[3 * k + 1] = vr[p].y; out.vel[3 * k + 2] = vr[p].z; }
    if (out.rhop) out.rhop[k] = vr[p].w;
    k++;
  }
  if (k != s.np) throw SphError(SPH_ERR_STATE, "owned particle count mismatch");
  out.n = k;
}

void SphGpuSingle::DownloadInteraction(SphInterOut& out) {
  if (slab()) throw SphError(SPH_ERR_UNSUPPORTED, "interaction download is single-domain only");
  // Runs one interaction on the current state (like or_interaction) and reads ar/ace back.
  // Maxima accumulated so far (VelMax from the last divide) are kept for this call.
  Interaction_Forces(1);
  // an inspection: the SPS stress tensor of the state stays the one the next step starts from
  if (sps_) std::swap(cur_.tau, taunew_);
  DtVariable(DT_PEEK);
  const SphRunStats s = Stats();
  const unsigned nheld = sc_host_->np;  // with periodic boundaries: the duplicates too
  std::vector<float4> a(nheld);
  check_hip(hipMemcpy(a.data(), arace_, 16 * size_t(nheld), hipMemcpyDeviceToHost), "download arace");
  std::vector<typecode> code;
  if (peri_) {
    code.resize(nheld);
    check_hip(hipMemcpy(code.data(), cur_.code, 2 * size_t(nheld), hipMemcpyDeviceToHost), "download code");
  }
  unsigned k = 0;
  for (unsigned p = 0; p < nheld; p++) {
    if (peri_ && !CodeIsNormal(code[p])) continue;  // normal particles, in device order
    if (k >= s.np) throw SphError(SPH_ERR_STATE, "normal particle count mismatch");
    if (out.ar) out.ar[k] = a[p].w;
    if (out.ace) { out.ace[3 * k] = a[p].x; out.ace[3 * k + 1] = a[p].y; out.ace[3 * k + 2] = a[p].z; }
    k++;
  }
  if (k != s.np) throw SphError(SPH_ERR_STATE, "normal particle count mismatch");
  out.velmax = s.velmax;
  out.acemax = s.acemax;
  out.viscdtmax = s.viscdtmax;
  // Leave the device maxima as a fresh interaction would find them (VelMax stays:
  // it belongs to the last divide).
  check_hip(hipMemsetAsync(&sc_->red[RED_ACEMAX2][0], 0, 4 * RED_SLOTS, stream), "reset acemax");
  check_hip(hipMemsetAsync(&sc_->red[RED_VISCDT][0], 0, 4 * RED_SLOTS, stream), "reset viscdt");
  Sync();
}

// The outputs of k_fluid_ext that DownloadInteraction does not show: the shifting sums and the
// SPS stress tensor of one Interaction_Forces(1) on the current state.
void SphGpuSingle::DownloadExt(SphExtOut& out, bool keep_tau) {
  if (slab()) throw SphError(SPH_ERR_UNSUPPORTED, "ext download is single-domain only");
  if (out.tau && !sps_) throw SphError(SPH_ERR_STATE, "the case has no Laminar+SPS viscosity (no SPS stress tensor)");
  if (out.shiftposfs && !shift_) throw SphError(SPH_ERR_STATE, "the case has no shifting (no shifting sums)");
  if (!ext_) throw SphError(SPH_ERR_STATE, "the case has neither Laminar+SPS viscosity nor shifting");
  Interaction_Forces(1);  // the new tensor is cur_.tau now, the one the pairs read taunew_
  Stats();  // waits for the interaction; the counts are in sc_host_
  const unsigned n = sc_host_->np, npb = sc_host_->npb;
  if (out.shiftposfs) {
    std::vector<float4> sp(n);
    check_hip(hipMemcpy(sp.data(), shiftpos_, 16 * size_t(n), hipMemcpyDeviceToHost), "download shiftposfs");
    for (unsigned p = 0; p < n; p++) {
      const float4 v = p < npb ? make_float4(0.f, 0.f, 0.f, 0.f) : sp[p];
      out.shiftposfs[4 * p] = v.x;
      out.shiftposfs[4 * p + 1] = v.y;
      out.shiftposfs[4 * p + 2] = v.z;
      out.shiftposfs[4 * p + 3] = v.w;
    }
  }
  if (out.tau) {
    std::vector<float4> t(2 * size_t(n));
    check_hip(hipMemcpy(t.data(), cur_.tau, 32 * size_t(n), hipMemcpyDeviceToHost), "download tau");
    for (unsigned p = 0; p < n; p++) {
      const float4 a = t[2 * size_t(p)], b = t[2 * size_t(p) + 1];
      const bool bound = p < npb;
      float* o = out.tau + 6 * size_t(p);
      o[0] = bound ? 0.f : a.x;
      o[1] = bound ? 0.f : a.y;
      o[2] = bound ? 0.f : a.z;
      o[3] = bound ? 0.f : a.w;
      o[4] = bound ? 0.f : b.x;
      o[5] = bound ? 0.f : b.y;
    }
  }
  // an inspection leaves the state's tensor the one the next step starts from
  if (sps_ && !keep_tau) std::swap(cur_.tau, taunew_);
  // the device maxima as a fresh interaction would find them (DownloadInteraction)
  check_hip(hipMemsetAsync(&sc_->red[RED_ACEMAX2][0], 0, 4 * RED_SLOTS, stream), "reset acemax");
  check_hip(hipMemsetAsync(&sc_->red[RED_VISCDT][0], 0, 4 * RED_SLOTS, stream), "reset viscdt");
  Sync();
}

unsigned SphGpuSingle::DownloadNormals(float* out, unsigned cap, int* usenormalsft) {
  if (!normal_) throw SphError(SPH_ERR_STATE, "the case has no mDBC normals");
  if (usenormalsft) *usenormalsft = ftnormals_ ? 1 : 0;
  if (!out) return nnormal_;
  if (cap < nnormal_) throw SphError(SPH_ERR_ARG, "normals buffer too small");
  Sync();
  std::vector<float4> v(nnormal_);
  check_hip(hipMemcpy(v.data(), normal_, sizeof(float4) * nnormal_, hipMemcpyDeviceToHost), "download normals");
  for (unsigned i = 0; i < nnormal_; i++) {
    out[3 * i] = v[i].x;
    out[3 * i + 1] = v[i].y;
    out[3 * i + 2] = v[i].z;
  }
  return nnormal_;
}

void SphGpuSingle::CountPairs(uint64_t out[6]) {
  check_hip(hipMemsetAsync(pairs_, 0, 8 * 6, stream), "memset pairs");
  launch_count_pairs(stream, cap_, sc_, poscell_, begincell_, G, K, pairs_);
  unsigned long long h[6];
  check_hip(hipMemcpyAsync(h, pairs_, 8 * 6, hipMemcpyDeviceToHost, stream), "read pairs");
  Sync();
  for (int i = 0; i < 6; i++) out[i] = h[i];
}

}  // namespace sphx
