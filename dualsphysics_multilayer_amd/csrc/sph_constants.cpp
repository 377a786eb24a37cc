// sph_constants.cpp — the constants, grids and slab partitions derived from a case: pure host
// arithmetic, no device call.
#include "sph_solver_impl.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace sphx {

// ---- JSph::ConfigConstants1/2 (JSph.cpp:1392-1457), ConfigCellDivision (:1772-1788),
//      map limits (:2062-2076), SelecDomain/CalcCellCode (:1794-1829, JDsDcell.cpp:30-69) ----
unsigned bits_for(unsigned v, unsigned minbits) {
  unsigned n = minbits;
  for (; v >> n; n++) {}
  return n;
}
static unsigned cell_code(unsigned nx, unsigned ny, unsigned nz) {
  unsigned sx = bits_for(nx, 2), sy = bits_for(ny, 2), sz = bits_for(nz, 2);
  const unsigned smin = sx + sy + sz;
  if (smin > 31) return 0;
  for (unsigned rest = 31 - smin; rest;) {
    if (rest) { sx++; rest--; }
    if (rest) { sy++; rest--; }
    if (rest) { sz++; rest--; }
  }
  return ((sx + 1) << 25) | (sy << 20) | (sz << 15) | ((sy + sz) << 10) | ((sx + 1 + sz) << 5) | (sx + 1 + sy);
}

void derive_constants(const SphCaseDef& c, SphConstants& k) {
  if (c.kernel != SPH_KERNEL_WENDLAND && c.kernel != SPH_KERNEL_CUBIC)
    throw SphError(SPH_ERR_ARG, "Kernel choice is not valid.");
  if (c.cellmode != SPH_CELLMODE_FULL && c.cellmode != SPH_CELLMODE_HALF) throw SphError(SPH_ERR_ARG, "invalid cellmode");
  if (c.step_algorithm != SPH_STEP_VERLET && c.step_algorithm != SPH_STEP_SYMPLECTIC)
    throw SphError(SPH_ERR_ARG, "invalid step algorithm");
  if (c.tdensity < 0 || c.tdensity > 3) throw SphError(SPH_ERR_ARG, "invalid DDT mode");
  if (c.npb > c.np) throw SphError(SPH_ERR_ARG, "npb > np");
  std::memset(&k, 0, sizeof(k));
  k.kernelh = float(c.h);
  k.cteb = float(c.cteb);
  k.gamma = float(c.gamma);
  k.rhopzero = float(c.rhop0);
  k.massfluid = float(c.massfluid);
  k.massbound = float(c.massbound);
  for (int i = 0; i < 3; i++) k.gravity[i] = float(c.gravity[i]);
  k.cflnumber = c.cflnumber;
  k.dp = c.dp;
  k.visco = float(c.visco);
  k.viscoboundfactor = float(c.viscoboundfactor);
  k.rhopoutmin = float(c.rhopoutmin);
  k.rhopoutmax = float(c.rhopoutmax);
  k.tdensity = c.tdensity;
  k.step_algorithm = c.step_algorithm;
  k.verlet_steps = c.verlet_steps;
  const double h = k.kernelh;
  k.kernelsize = float(h * 2.0f);  // Wendland factor 2 (FunSphKernel.h:190)
  k.kernelsize2 = k.kernelsize * k.kernelsize;
  k.data2d = c.data2d ? 1 : 0;
  if (k.data2d) {  // GetKernelWendland_Ctes(sim2d) (FunSphKernel.h:193-196)
    k.awen = float(0.557 / (h * h));
    k.bwen = float(-2.7852 / (h * h * h));
  } else {
    k.awen = float(0.41778 / (h * h * h));
    k.bwen = float(-2.08891 / (h * h * h * h));
  }
  k.kernel = c.kernel;
  if (k.kernel == SPH_KERNEL_CUBIC) {  // GetKernelCubic_Ctes (FunSphKernel.h:51-84)
    const double pi = 3.14159265358979323846;  // TypesDef.h:24
    const double a1 = k.data2d ? 10. / (pi * 7.) : 1. / pi;
    const double a2 = k.data2d ? a1 / (h * h) : a1 / (h * h * h);
    const double aa = k.data2d ? a1 / (h * h * h) : a1 / (h * h * h * h);
    const double deltap = 1. / 1.5;
    const double wdeltap = a2 * (1. - 1.5 * deltap * deltap + 0.75 * deltap * deltap * deltap);
    k.cub_od_wdeltap = float(1. / wdeltap);
    k.cub_a1 = float(a1);
    k.cub_a2 = float(a2);
    k.cub_aa = float(aa);
    k.cub_a24 = float(0.25 * a2);
    k.cub_c1 = float(-3. * aa);
    k.cub_d1 = float(9. * aa / 4.);
    k.cub_c2 = float(-3. * aa / 4.);
  }
  k.cs0 = std::sqrt(double(k.gamma) * double(k.cteb) / double(k.rhopzero));
  k.eta2 = float((h * 0.1) * (h * 0.1));
  k.ovrhopzero = 1.0f / k.rhopzero;
  k.ddtkh = k.kernelsize * float(c.ddtvalue);
  k.ddtgz = float(double(k.rhopzero) * double(std::fabs(k.gravity[2])) / double(k.cteb));
  k.dtini = c.dtini ? c.dtini : k.kernelh / k.cs0;
  k.dtmin = c.dtmin ? c.dtmin : (k.kernelh / k.cs0) * float(c.coefdtmin);
  k.scelldiv = (c.cellmode == SPH_CELLMODE_HALF ? 2 : 1);  // cells of 2h (full) or h (half)
  k.scell = k.kernelsize / k.scelldiv;
  k.movlimit = k.scell * 0.9f;
  // Periodic boundaries (JSph.cpp:718-730, 2067-2076): the own-axis component of each Peri?inc
  // is -MapRealSize, the cell map is the real map widened by KernelSize on each periodic axis
  if (c.peri_active < 0 || c.peri_active > 7) throw SphError(SPH_ERR_ARG, "invalid peri_active");
  k.peri_active = c.peri_active;
  if (k.peri_active) {
    if (k.data2d && (k.peri_active & 2)) throw SphError(SPH_ERR_ARG, "Cannot use periodic conditions in Y with 2D simulations");
    if (c.symmetry && (k.peri_active & 2))
      throw SphError(SPH_ERR_ARG, "Symmetry is not allowed with periodic conditions in axis Y.");
  }
  for (int i = 0; i < 3; i++) {
    k.map_realposmin[i] = c.map_realposmin[i];
    k.map_realsize[i] = c.map_realposmax[i] - c.map_realposmin[i];
    if (!(k.map_realsize[i] > 0)) throw SphError(SPH_ERR_ARG, "invalid map limits");
    const bool peri = (k.peri_active >> i) & 1;
    const double pmin = peri ? c.map_realposmin[i] - double(k.kernelsize) : c.map_realposmin[i];
    const double pmax = peri ? c.map_realposmax[i] + double(k.kernelsize) : c.map_realposmax[i];
    k.dom_posmin[i] = pmin;
    // (without periodic axes Map_Size is MapRealSize, the value used before they existed, and
    // map_posmin / map_posmax stay zero: the map is the real map)
    const double mapsize = peri ? pmax - pmin : k.map_realsize[i];
    if (k.peri_active) {
      k.map_posmin[i] = pmin;
      k.map_posmax[i] = pmax;
    }
    k.dom_cells[i] = unsigned(std::ceil(mapsize / k.scell));
    // a period of at most 2 KernelSize would make a particle a neighbour of its own image, and
    // the duplicates of one pass would not be the whole rim (not a case the reference foresees)
    if (peri && !(k.map_realsize[i] > 2.0 * double(k.kernelsize)))
      throw SphError(SPH_ERR_ARG, "periodic boundaries: a periodic axis must be longer than twice the interaction distance");
    if (peri) {
      const double* in = (i == 0 ? c.peri_xinc : i == 1 ? c.peri_yinc : c.peri_zinc);
      double* out = (i == 0 ? k.peri_xinc : i == 1 ? k.peri_yinc : k.peri_zinc);
      for (int j = 0; j < 3; j++) out[j] = in[j];
      out[i] = -k.map_realsize[i];
    }
  }
  k.dom_cellcode = cell_code(k.dom_cells[0] + 1, k.dom_cells[1] + 1, k.dom_cells[2] + 1);
  if (!k.dom_cellcode) throw SphError(SPH_ERR_ARG, "failed to select a valid CellCode");
  // Boundary configuration (JSph.cpp:626-640, 785-790).
  k.tboundary = (c.tboundary == 0 ? SPH_BOUND_DBC : c.tboundary);
  if (k.tboundary != SPH_BOUND_DBC && k.tboundary != SPH_BOUND_MDBC)
    throw SphError(SPH_ERR_ARG, "Boundary Condition method is not valid.");
  k.slipmode = (k.tboundary == SPH_BOUND_MDBC ? (c.slipmode == 0 ? SPH_SLIP_VEL0 : c.slipmode) : SPH_SLIP_VEL0);
  if (k.slipmode != SPH_SLIP_VEL0)
    throw SphError(SPH_ERR_UNSUPPORTED, "Only the slip mode velocity=0 is allowed with mDBC conditions.");
  k.mdbc_threshold = (k.tboundary == SPH_BOUND_MDBC ? float(c.mdbc_threshold) : 0.f);
  // Rheology, viscosity and shifting options (JSph::LoadConfigParameters, JSph.cpp:608-700 of
  // the v5.0 solver; JSph.cpp:620-700 of v5.2).
  k.rheology = (c.rheology == 0 ? SPH_RHEOLOGY_SINGLE : c.rheology);
  k.velgrad = (c.velgrad == 0 ? SPH_VELGRAD_FDA : c.velgrad);
  k.tvisco = (c.tvisco == 0 ? SPH_VISCO_ARTIFICIAL : c.tvisco);
  k.shift_mode = c.shift_mode;
  k.shift_coef = float(c.shift_coef);
  k.shift_tfs = float(c.shift_tfs);
  k.relaxation_dt = float(c.relaxation_dt);
  if (k.rheology != SPH_RHEOLOGY_SINGLE && k.rheology != SPH_RHEOLOGY_NN)
    throw SphError(SPH_ERR_ARG, "Rheology treatment is not valid.");
  if (k.velgrad != SPH_VELGRAD_FDA && k.velgrad != SPH_VELGRAD_SPH)
    throw SphError(SPH_ERR_ARG, "Velocity gradient treatment is not valid.");
  if (k.tvisco < SPH_VISCO_ARTIFICIAL || k.tvisco > SPH_VISCO_CONSTEQ)
    throw SphError(SPH_ERR_ARG, "Viscosity treatment is not valid.");
  if (k.shift_mode < SPH_SHIFT_NONE || k.shift_mode > SPH_SHIFT_FULL)
    throw SphError(SPH_ERR_ARG, "Shifting mode is not valid.");
  k.dtallparticles = c.dtallparticles ? 1 : 0;  // JSph.cpp:697
  // Symmetry (JSph.cpp:714; its checks :1174-1179, MapRealPosMin.y = 0 :1386)
  k.symmetry = c.symmetry ? 1 : 0;
  if (k.symmetry) {
    if (k.data2d) throw SphError(SPH_ERR_ARG, "Symmetry is not allowed with 2-D simulations.");
    if (k.tvisco != SPH_VISCO_ARTIFICIAL) throw SphError(SPH_ERR_ARG, "Symmetry is only allowed with Artificial viscosity.");
    if (c.map_realposmin[1] != 0.0) throw SphError(SPH_ERR_ARG, "Symmetry needs MapRealPosMin.y = 0 (JSph.cpp:1386)");
    if (k.rheology != SPH_RHEOLOGY_SINGLE)
      throw SphError(SPH_ERR_UNSUPPORTED, "Symmetry is implemented for the single-phase interaction");
  }
  if (!(c.dtfixed >= 0)) throw SphError(SPH_ERR_ARG, "DtFixed must not be negative");
  k.dtfixed = c.dtfixed;  // max(0, DtFixed), JSph.cpp:699
  if (k.rheology == SPH_RHEOLOGY_SINGLE) {
    if (k.tvisco == SPH_VISCO_CONSTEQ)
      throw SphError(SPH_ERR_ARG, "ViscoTreatment 'Constitutive  eq.' not valid for Single-phase classic formulation.");
    if (k.tvisco == SPH_VISCO_LAMINARSPS) {  // JSph::ConfigConstants2 (JSph.cpp:1438-1443)
      const double dp_sps = (k.data2d ? std::sqrt(c.dp * c.dp * 2.) / 2. : std::sqrt(c.dp * c.dp * 3.) / 3.);
      k.spssmag = float(std::pow(0.12 * dp_sps, 2));
      k.spsblin = float((2. / 3.) * 0.0066 * dp_sps * dp_sps);
    }
    return;
  }
  // NN multiphase: JSph::InitMultiPhase + ConfigConstantsMP (JSph.cpp:3137-3242, v5.0 solver)
  if (k.tboundary == SPH_BOUND_MDBC)
    throw SphError(SPH_ERR_ARG, "Multiphase formulations are not supported with BC_mDBC.");
  if (c.nphases < 1 || c.nphases > SPH_MAXPHASES) throw SphError(SPH_ERR_ARG, "The number of phases is invalid.");
  k.nphases = c.nphases;
  bool cs0_present = true;
  for (unsigned p = 0; p < c.nphases; p++) {
    if (c.phases[p].phasetype != 0) throw SphError(SPH_ERR_UNSUPPORTED, "only phasetype 0 (non-Newtonian) exists in v5.0");
    if (p && c.phases[p].mkfluid <= c.phases[p - 1].mkfluid)
      throw SphError(SPH_ERR_ARG, "phases must be sorted by mkfluid");
    if (!float(c.phases[p].cs0)) cs0_present = false;
  }
  for (unsigned p = 0; p < c.nphases; p++) {
    const SphPhaseDef& ph = c.phases[p];
    const float rho = float(ph.rho), gam = (float(ph.gamma) ? float(ph.gamma) : k.gamma), cs = float(ph.cs0);
    k.phase_mass[p] = float(double(rho) * (k.data2d ? c.dp * c.dp : c.dp * c.dp * c.dp));
    // with a <csound> for every phase: CteB of InitMultiPhase (float arithmetic), else from
    // the case's Cs0 (ConfigConstantsMP, double arithmetic)
    k.phase_cteb[p] = cs0_present ? cs * cs * rho / gam : float(k.cs0 * k.cs0 * double(rho) / double(gam));
  }
  // DtMin is set here whatever the XML gives (ConfigConstantsMP runs after the parameters
  // are read, and ConfigConstants2 keeps a non-zero DtMin)
  const float coefdtmin = float(c.coefdtmin) * 1.0e-5f;  // CoefDtMin*=1.0e-5f
  k.dtmin = (double(k.kernelh) / k.cs0) * double(coefdtmin);
}

KConst make_kconst(const SphConstants& c) {
  KConst K;
  std::memset(&K, 0, sizeof(K));
  K.kernelh = c.kernelh;
  K.kernelsize2 = c.kernelsize2;
  K.bwen = c.bwen;
  K.ovkernelh = 1.0f / c.kernelh;
  K.cteb = c.cteb;
  K.gamma = c.gamma;
  K.rhopzero = c.rhopzero;
  K.ovrhopzero = c.ovrhopzero;
  K.massfluid = c.massfluid;
  K.massbound = c.massbound;
  K.eta2 = c.eta2;
  K.ddtkh = c.ddtkh;
  K.ddtgz = c.ddtgz;
  K.cs0f = float(c.cs0);
  K.visco = c.visco;
  K.viscobound = c.visco * c.viscoboundfactor;
  K.scell = c.scell;
  K.movlimit = c.movlimit;
  K.rhopoutmin = c.rhopoutmin;
  K.rhopoutmax = c.rhopoutmax;
  K.gravx = c.gravity[0];
  K.gravy = c.gravity[1];
  K.gravz = c.gravity[2];
  K.ovgamma = 1.f / c.gamma;
  K.gravxd = c.gravity[0];
  K.gravyd = c.gravity[1];
  K.gravzd = c.gravity[2];
  K.map_realposmin_x = c.map_realposmin[0];
  K.map_realposmin_y = c.map_realposmin[1];
  K.map_realposmin_z = c.map_realposmin[2];
  K.map_realsize_x = c.map_realsize[0];
  K.map_realsize_y = c.map_realsize[1];
  K.map_realsize_z = c.map_realsize[2];
  K.scelld = double(c.scell);
  K.domcellcode = c.dom_cellcode;
  K.tdensity = c.tdensity;
  K.mhalfovh = -0.5f * K.ovkernelh;
  K.bwenovh = c.bwen * K.ovkernelh;
  // Cubic spline (FunSphKernel.h:38-175): the tiled kernels evaluate its fac directly, so
  // the per-pass factor the Wendland (bwen/h) takes is 1
  K.cubic = (c.kernel == SPH_KERNEL_CUBIC) ? 1 : 0;
  K.kfold = K.cubic ? 1.f : K.bwenovh;
  K.cub_a2 = c.cub_a2;
  K.cub_a24 = c.cub_a24;
  K.cub_c1 = c.cub_c1;
  K.cub_d1 = c.cub_d1;
  K.cub_c2 = c.cub_c2;
  K.cub_odw = c.cub_od_wdeltap;
  K.ddtkhcs = c.ddtkh * K.cs0f;
  K.awen = c.awen;
  K.mdbc = (c.tboundary == SPH_BOUND_MDBC) ? 1 : 0;
  K.scelldiv = c.scelldiv;
  {  // SPH_TILE_FULL=1 (test hook, read once): the tiled kernels' full test groups and rounds of 128
    static const bool full = [] {
      const char* e = std::getenv("SPH_TILE_FULL");
      return e && std::atoi(e) != 0;
    }();
    if (full) test_hook_notice("SPH_TILE_FULL");
    K.tilefull = full ? 1 : 0;
  }
  K.nn =(c.rheology == SPH_RHEOLOGY_NN) ? 1 : 0;
  K.nntvisco = c.tvisco;
  K.nnvelgrad = c.velgrad;
  K.tvisco = c.tvisco;
  K.spssmag = c.spssmag;
  K.spsblin = c.spsblin;
  K.shiftmode = c.shift_mode;
  K.sim2d = c.data2d;
  K.lamda = c.relaxation_dt;
  K.shifttfs = c.shift_tfs;
  K.shiftcoef = c.shift_coef;
  K.shiftmaxdist = float(c.dp * 0.1);
  K.coeftfs = (c.data2d ? 2.0 : 3.0) - double(c.shift_tfs);
  K.dtallp = c.dtallparticles;
  K.symmetry = c.symmetry;
  K.dtfix_val = c.dtfixed;
  K.viscobf = c.viscoboundfactor;
  {  // binomial coefficients of (1+x)^(1/gamma) - 1
    const double a = 1.0 / double(c.gamma);
    K.ddtc1 = float(a);
    K.ddtc2 = float(a * (a - 1) / 2);
    K.ddtc3 = float(a * (a - 1) * (a - 2) / 6);
    K.ddtc4 = float(a * (a - 1) * (a - 2) * (a - 3) / 24);
    // |drz| <= 2h for every pair, so the series applies to all pairs of the case when
    // 2h*ddtgz is small (dam break: ~1e-3); decided once here, uniform in the kernel.
    // three terms: the x^4 term is 0.19 x^3 of the first, < 2e-6 for x < 0.02 (sph_interaction_tiled.hip)
    K.ddtseries = (double(c.kernelsize) * double(c.ddtgz) < 0.02) ? 1 : 0;
    const double gz = double(c.ddtgz), r0 = double(c.rhopzero);
    K.ddte1 = float(r0 * a * gz);
    K.ddte2 = float(r0 * a * (a - 1) / 2 * gz * gz);
    K.ddte3 = float(r0 * a * (a - 1) * (a - 2) / 6 * gz * gz * gz);
    K.ddte4 = float(r0 * a * (a - 1) * (a - 2) * (a - 3) / 24 * gz * gz * gz * gz);
  }
  return K;
}

PeriConst make_periconst(const SphConstants& c) {
  PeriConst P;
  std::memset(&P, 0, sizeof(P));
  P.active = c.peri_active;
  for (int i = 0; i < 3; i++) {
    P.cellmax[i] = c.dom_cells[i] ? c.dom_cells[i] - 1u : 0u;
    P.inc[0][i] = c.peri_xinc[i];
    P.inc[1][i] = c.peri_yinc[i];
    P.inc[2][i] = c.peri_zinc[i];
    P.domposmin[i] = c.dom_posmin[i];
    P.mapposmin[i] = c.map_posmin[i];
    P.mapposmax[i] = c.map_posmax[i];
  }
  return P;
}

// RunPeriodic on the host for the initial particles (JSphCpuSingle.cpp:361-431, counts only):
// the duplicates of the first divide, which size the particle capacity.
unsigned initial_periodic_count(const SphConstants& C, const SphParticlesHost& h, unsigned npb) {
  const PeriConst P = make_periconst(C);
  struct V3 { double x, y, z; };
  auto inside = [&](const V3& q) {
    return P.mapposmin[0] <= q.x && P.mapposmin[1] <= q.y && P.mapposmin[2] <= q.z && q.x < P.mapposmax[0] &&
           q.y < P.mapposmax[1] && q.z < P.mapposmax[2];
  };
  unsigned long long total = 0;
  for (int type = 0; type < 2; type++) {
    std::vector<V3> made;  // the type's new duplicates, in list order
    const unsigned p0 = type ? npb : 0u, p1 = type ? h.n : npb;
    for (int ax = 0; ax < 3; ax++) {
      if (!(P.active & (1 << ax))) continue;
      const V3 inc{P.inc[ax][0], P.inc[ax][1], P.inc[ax][2]};
      std::vector<V3> add;
      auto list = [&](const V3& q) {
        const V3 a{q.x + inc.x, q.y + inc.y, q.z + inc.z}, b{q.x - inc.x, q.y - inc.y, q.z - inc.z};
        if (inside(a)) add.push_back(a);
        if (inside(b)) add.push_back(b);
      };
      for (const V3& q : made) list(q);
      for (unsigned p = p0; p < p1; p++) list(V3{h.pos[3 * p], h.pos[3 * p + 1], h.pos[3 * p + 2]});
      made.insert(made.end(), add.begin(), add.end());
    }
    total += made.size();
  }
  if (total > 0x7fffffffull) throw SphError(SPH_ERR_ARG, "The number of particles is too big.");
  return unsigned(total);
}

// Ghost columns per slab face: the support radius 2h is one full cell or two half cells
// (scelldiv); with mDBC one column more, because a boundary particle's ghost node lies up
// to |2 normal| (about dp, less than a cell) from it and its search reaches 2h around the
// node (JSphCpu.cpp:1040-1047): a slab owning such a particle in its face column needs the
// fluid one column beyond.
int ghost_width(const SphConstants& c) { return int(c.scelldiv) + (c.tboundary == SPH_BOUND_MDBC ? 1 : 0); }

// Narrowest slab with neighbours on both sides: 2W columns, so that its two face column
// sets are disjoint.  A particle arriving from a neighbour (< one cell of movement) then
// lands in the face towards that neighbour, which keeps it as a ghost itself; in a narrower
// slab it could land in the opposite face and be missing from the other neighbour's ghosts
// until the next exchange.  A slab at the end of the map (one neighbour) needs W.
int min_slab_width(const SphConstants& c) { return 2 * ghost_width(c); }

// Full-map cell grid (JCellDivCpuSingle::PrepareNct, JCellDivCpuSingle.cpp:105-121, with CellDomFixed).
// A slab keeps the global extent of the other two axes and the cells [c0-W, c1+W) of its
// slab axis (owned + W ghost cells per face, W = ghost_width).
DivGrid make_grid(const SphConstants& c, const SlabConfig* slab) {
  DivGrid g;
  g.ncx = int(c.dom_cells[0]);
  g.ncy = int(c.dom_cells[1]);
  g.ncz = int(c.dom_cells[2]);
  g.axis = 0;
  g.soff = 0;
  g.sown0 = 0;
  g.sown1 = g.ncx;
  if (slab) {
    const int W = ghost_width(c);
    const bool both = slab->rank > 0 && slab->rank + 1 < slab->nranks;
    if (slab->axis != 0 && slab->axis != 1) throw SphError(SPH_ERR_ARG, "slab axis must be 0 (x) or 1 (y)");
    const int ext = slab->axis ? g.ncy : g.ncx;
    if (slab->nranks < 1 || slab->rank < 0 || slab->rank >= slab->nranks || slab->c0 < 0 ||
        slab->c1 < slab->c0 + (both ? min_slab_width(c) : W) || slab->c1 > ext)
      throw SphError(SPH_ERR_ARG,
                     "invalid slab cells (a slab owns at least 2W cells of its axis, W at a map end; W = the ghost "
                     "width: scelldiv cells, +1 with mDBC)");
    g.axis = slab->axis;
    g.soff = slab->c0 - W;
    (slab->axis ? g.ncy : g.ncx) = slab->c1 - slab->c0 + 2 * W;
    g.sown0 = W;
    g.sown1 = W + slab->c1 - slab->c0;
  }
  g.nsheet = unsigned(g.ncx) * unsigned(g.ncy);
  const unsigned long long nct = (unsigned long long)g.nsheet * unsigned(g.ncz);
  if (nct * 2 + 7 >= (1ull << 31)) throw SphError(SPH_ERR_ARG, "the number of cells is too big");
  g.nct = unsigned(nct);
  g.boxboundignore = g.nct;
  g.boxfluid = g.boxboundignore + 1;
  g.boxboundout = g.boxfluid + g.nct;
  g.boxfluidout = g.boxboundout + 1;
  g.boxboundoutignore = g.boxfluidout + 1;
  g.boxfluidoutignore = g.boxboundoutignore + 1;
  g.boxdiscard = g.boxfluidoutignore + 1;
  g.nctt = g.nct * 2 + 6;
  return g;
}

// Global cell of every initial particle along `axis` (JSph::LoadDcellParticles, JSph.cpp:1690-1711).
std::vector<unsigned> initial_columns(const SphConstants& C, const SphParticlesHost& h, int axis) {
  std::vector<unsigned> cx(h.n);
  for (unsigned p = 0; p < h.n; p++) {
    const double dx = h.pos[3 * p + axis] - C.dom_posmin[axis];
    cx[p] = dx >= 0 ? unsigned(dx / double(C.scell)) : 0u;
  }
  return cx;
}

// Contiguous split of the columns into nranks slabs of at least minw columns that
// minimises the heaviest slab (the step time of the slowest rank): bisection on the load
// bound L, each bound probed greedily (every slab takes columns while it stays <= L and
// leaves minw columns for each slab after it).  Falls back to the prefix quantiles when no
// bound is feasible (a slab of minw columns already exceeds every L tried).  cfg3 on 8
// ranks: heaviest slab 1.33M -> 1.21M particles (quantile cuts at whole columns of 143k /
// 190k particles had given one rank an extra column).
static bool greedy_split(const std::vector<double>& pre, int nranks, int minw, double L, int* b) {
  const int ncx = int(pre.size()) - 1;
  b[0] = 0;
  for (int r = 0; r < nranks - 1; r++) {
    const int lo = b[r] + minw, hi = ncx - (nranks - 1 - r) * minw;
    if (lo > hi || pre[size_t(lo)] - pre[size_t(b[r])] > L) return false;
    int e = lo;
    while (e < hi && pre[size_t(e) + 1] - pre[size_t(b[r])] <= L) e++;
    b[r + 1] = e;
  }
  b[nranks] = ncx;
  return pre[size_t(ncx)] - pre[size_t(b[nranks - 1])] <= L && ncx - b[nranks - 1] >= minw;
}

void partition_from_prefix(const std::vector<double>& pre, int nranks, int* b, int minw) {
  const int ncx = int(pre.size()) - 1;
  const double total = pre[size_t(ncx)];
  double lo = total / double(nranks), hi = total;
  std::vector<int> best(size_t(nranks) + 1, -1), t(size_t(nranks) + 1);
  if (greedy_split(pre, nranks, minw, hi, t.data())) best = t;
  for (int it = 0; it < 60 && best[0] == 0; it++) {
    const double mid = 0.5 * (lo + hi);
    if (greedy_split(pre, nranks, minw, mid, t.data())) {
      best = t;
      hi = mid;
    } else {
      lo = mid;
    }
  }
  if (best[0] == 0) {
    for (int r = 0; r <= nranks; r++) b[r] = best[size_t(r)];
    return;
  }
  // no feasible bound: the prefix quantiles, clamped to the minimum width
  b[0] = 0;
  b[nranks] = ncx;
  int c = 0;
  for (int r = 1; r < nranks; r++) {
    const double target = total * double(r) / double(nranks);
    while (c < ncx && pre[size_t(c)] < target) c++;
    int cut = c;
    if (cut > 0 && target - pre[size_t(cut) - 1] < pre[size_t(cut)] - target) cut--;
    cut = std::max(cut, b[r - 1] + minw);
    cut = std::min(cut, ncx - (nranks - r) * minw);
    b[r] = cut;
  }
}

void slab_partition(const SphCaseDef& cdef, const SphParticlesHost& all, int nranks, double bound_weight, int* b,
                    int axis) {
  SphConstants C;
  derive_constants(cdef, C);
  if (axis != 0 && axis != 1) throw SphError(SPH_ERR_ARG, "slab axis must be 0 (x) or 1 (y)");
  const int ncx = int(C.dom_cells[axis]), W = min_slab_width(C);
  if (nranks < 1 || (nranks > 1 && nranks * W > ncx))
    throw SphError(SPH_ERR_ARG, "nranks must be in [1, cells of the slab axis / (2 x ghost width)]");
  if (all.n != cdef.np) throw SphError(SPH_ERR_ARG, "particle count does not match the case");
  std::vector<double> w(size_t(ncx), 0.0);
  const std::vector<unsigned> cx = initial_columns(C, all, axis);
  for (unsigned p = 0; p < all.n; p++) w[std::min<unsigned>(cx[p], unsigned(ncx - 1))] += (p < cdef.npb ? bound_weight : 1.0);
  std::vector<double> pre(size_t(ncx) + 1, 0.0);
  for (int c = 0; c < ncx; c++) pre[size_t(c) + 1] = pre[size_t(c)] + w[size_t(c)];
  partition_from_prefix(pre, nranks, b, W);
}

}  // namespace sphx
