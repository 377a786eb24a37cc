// sph_solver_inout.cpp — SphGpuSingle: inlet/outlet zones (sph_inout.hip).
#include "sph_solver.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace sphx {

// ---- inlet/outlet zones (sph_inout.hip) --------------------------------------------------------
// InitCheckProximity (JSphInOut.cpp:704-775) of the new inout particles `npos` against each
// other and the particles held (pxy, pz, code; in device order): a normal fluid particle too
// close to one is excluded (its code changed), anything else too close refuses the zones.
static void inout_check_proximity(double dp, const std::vector<double>& npos, const std::vector<double2>& pxy,
                                  const std::vector<double>& pz, std::vector<typecode>& code) {
  const unsigned nnew = unsigned(npos.size() / 3), n = unsigned(code.size());
  const double dist = dp * 0.8, dist2 = dist * dist;
  double lo[3] = {npos[0], npos[1], npos[2]};
  for (unsigned q = 0; q < nnew; q++)
    for (int i = 0; i < 3; i++) lo[i] = std::min(lo[i], npos[3 * size_t(q) + i]);
  for (int i = 0; i < 3; i++) lo[i] -= 2 * dist;
  auto cellkey = [&](long long cx, long long cy, long long cz) -> unsigned long long {
    return ((unsigned long long)(cx & 0x1fffff) << 42) | ((unsigned long long)(cy & 0x1fffff) << 21) |
           (unsigned long long)(cz & 0x1fffff);
  };
  std::unordered_map<unsigned long long, std::vector<unsigned>> grid;
  auto cellof = [&](const double* p, long long c[3]) {
    for (int i = 0; i < 3; i++) c[i] = (long long)std::floor((p[i] - lo[i]) / dist);
  };
  for (unsigned q = 0; q < nnew; q++) {
    long long c[3];
    cellof(&npos[3 * size_t(q)], c);
    grid[cellkey(c[0], c[1], c[2])].push_back(q);
  }
  auto near = [&](const double* p, unsigned self) -> bool {
    long long c[3];
    cellof(p, c);
    if (c[0] < -1 || c[1] < -1 || c[2] < -1 || c[0] > 0xfffff || c[1] > 0xfffff || c[2] > 0xfffff) return false;
    for (long long x = c[0] - 1; x <= c[0] + 1; x++)
      for (long long y = c[1] - 1; y <= c[1] + 1; y++)
        for (long long zc = c[2] - 1; zc <= c[2] + 1; zc++) {
          const auto it = grid.find(cellkey(x, y, zc));
          if (it == grid.end()) continue;
          for (unsigned q : it->second) {
            if (q == self) continue;
            const double ddx = p[0] - npos[3 * size_t(q)], ddy = p[1] - npos[3 * size_t(q) + 1],
                         ddz = p[2] - npos[3 * size_t(q) + 2];
            if (ddx * ddx + ddy * ddy + ddz * ddz <= dist2) return true;
          }
        }
    return false;
  };
  unsigned nerr = 0;
  for (unsigned q = 0; q < nnew; q++) nerr += near(&npos[3 * size_t(q)], q) ? 1u : 0u;
  for (unsigned p = 0; p < n; p++) {
    const double pp[3] = {pxy[p].x, pxy[p].y, pz[p]};
    if (!CodeIsNormal(code[p]) || !near(pp, ~0u)) continue;
    if (CodeIsFluid(code[p])) code[p] = CodeSetNormal(code[p]) | CODE_OUTIGNORE;  // excluded fluid
    else nerr++;
  }
  if (nerr)
    throw SphError(SPH_ERR_ARG, "There are inout fluid or boundary particles too close to inout particles.");
}

// JSphCpuSingle::InOutInit (JSphCpuSingle_InOut.cpp:72-137).
void SphGpuSingle::SetInOut(const SphInOutDef& def, const SphInOutZoneDef* zones, const double* points,
                            unsigned npoints) {
  if (inout_) throw SphError(SPH_ERR_STATE, "the inlet/outlet zones are already configured");
  if (stepped_) throw SphError(SPH_ERR_STATE, "configure the inlet/outlet zones before the first step");
  if (slab()) throw SphError(SPH_ERR_UNSUPPORTED, "inlet/outlet zones are not implemented for slab solvers");
  const char* bad = nullptr;
  if (peri_) bad = "periodic boundaries";
  else if (C.tboundary == SPH_BOUND_MDBC) bad = "mDBC";
  else if (nn_) bad = "NN multiphase";
  else if (sps_ || shift_) bad = "Laminar+SPS or shifting";
  else if (C.symmetry) bad = "Symmetry";
  else if (nftbodies_ || nmotobj_) bad = "moving boundaries or floating bodies";
  else if (gauges_.ng) bad = "gauges";
  else if (C.kernel == SPH_KERNEL_CUBIC) bad = "the Cubic spline kernel";
  if (bad) throw SphError(SPH_ERR_UNSUPPORTED, std::string("inlet/outlet zones with ") + bad + " are not implemented");
  if (def.nzones < 1 || def.nzones > unsigned(INOUT_MAXZONES))
    throw SphError(SPH_ERR_ARG, "Maximum number of inlet/outlet zones has been reached.");
  if (def.extrapolatemode < 1 || def.extrapolatemode > 3) throw SphError(SPH_ERR_ARG, "invalid extrapolatemode");
  check_hip(hipSetDevice(device), "hipSetDevice");
  const SphRunStats st = Stats();
  if (st.nstep || st.time != 0) throw SphError(SPH_ERR_UNSUPPORTED, "Simulation restart not allowed when Inlet/Outlet is used.");
  const unsigned n = sc_host_->np;
  // -- the zone data
  InOutDev io;
  std::memset(&io, 0, sizeof(io));
  io.nzones = int(def.nzones);
  io.useboxlimit = def.useboxlimit != 0;
  io.checkfreelimit = (def.useboxlimit != 0 && def.nzones > 2);  // JSphInOut.cpp:807
  io.extrapmode = def.extrapolatemode;
  io.determlimit = def.determlimit;
  io.coefhydro = K.rhopzero * (-K.gravz) / K.cteb;  // JSphInOut.cpp:536
  io.codenewpart = def.codenewpart;
  if (CodeType(typecode(def.codenewpart)) != CODE_TYPE_FLUID || CodeIsFluidInout(typecode(def.codenewpart)))
    throw SphError(SPH_ERR_ARG, "There are not free fluid codes for new particles created during the simulation.");
  for (int i = 0; i < 3; i++) {
    io.freemin[i] = def.freelimitmin[i];
    io.freemax[i] = def.freelimitmax[i];
  }
  std::vector<double> npos;  // the initial inout particles (LoadInitPartsData, JSphInOut.cpp:675-695)
  std::vector<typecode> ncode;
  for (unsigned c = 0; c < def.nzones; c++) {
    const SphInOutZoneDef& z = zones[c];
    InOutZoneDev& d = io.z[c];
    if ((z.cfgzone & IO_VELM_MASK) != IO_VELM_FIXED && (z.cfgzone & IO_VELM_MASK) != IO_VELM_EXTRAPOLATED)
      throw SphError(SPH_ERR_UNSUPPORTED, "inlet/outlet zones: variable and interpolated velocities are not implemented");
    if ((z.cfgzone & IO_RHOP_MASK) > IO_RHOP_EXTRAPOLATED) throw SphError(SPH_ERR_ARG, "inlet/outlet zone: invalid density mode");
    if (z.cfgupdate & IO_REFILLADVANCED)
      throw SphError(SPH_ERR_UNSUPPORTED, "inlet/outlet zones: the advanced refilling is not implemented");
    if (z.layers < 1 || z.layers > 250) throw SphError(SPH_ERR_ARG, "inlet/outlet zone: layers must be in [1, 250]");
    if (size_t(z.point0) + z.npoints > npoints) throw SphError(SPH_ERR_ARG, "inlet/outlet zone: points out of range");
    for (int i = 0; i < 4; i++) {
      d.plane[i] = z.plane[i];
      d.vel0[i] = z.veldata[0][i];
    }
    for (int i = 0; i < 3; i++) {
      d.dir[i] = float(z.direction[i]);
      d.boxmin[i] = z.boxlimitmin[i];
      d.boxmax[i] = z.boxlimitmax[i];
    }
    d.width = z.width;
    d.zsurf = z.zsurf;
    d.cfgzone = z.cfgzone;
    d.cfgupdate = z.cfgupdate;
    for (unsigned layer = 0; layer < z.layers; layer++) {
      const double f = -C.dp * double(layer);
      const double dx = z.direction[0] * f, dy = z.direction[1] * f, dz = z.direction[2] * f;
      for (unsigned q = 0; q < z.npoints; q++) {
        const double* pt = points + 3 * (size_t(z.point0) + q);
        const double pp[3] = {pt[0] + dx, pt[1] + dy, pt[2] + dz};
        for (int i = 0; i < 3; i++) {
          const double r = pp[i] - C.dom_posmin[i];
          if (!(r >= 0 && r < C.map_realsize[i]))
            throw SphError(SPH_ERR_ARG, "Point for inlet conditions is outside the domain.");
          npos.push_back(pp[i]);
        }
        ncode.push_back(typecode(CODE_TYPE_FLUID_INOUT + c));
      }
    }
  }
  const unsigned nnew = unsigned(ncode.size());
  if (!nnew) throw SphError(SPH_ERR_ARG, "inlet/outlet zones without initial particles");
  // -- InitCheckProximity (JSphInOut.cpp:704-775) against the particles held, in device order
  std::vector<double2> pxy(n);
  std::vector<double> pz(n);
  std::vector<typecode> code(n);
  check_hip(hipMemcpy(pxy.data(), cur_.posxy, 16 * size_t(n), hipMemcpyDeviceToHost), "download posxy");
  check_hip(hipMemcpy(pz.data(), cur_.posz, 8 * size_t(n), hipMemcpyDeviceToHost), "download posz");
  check_hip(hipMemcpy(code.data(), cur_.code, 2 * size_t(n), hipMemcpyDeviceToHost), "download code");
  inout_check_proximity(C.dp, npos, pxy, pz, code);
  // -- the capacity, fixed from here on (every check is done: nothing below refuses the zones)
  unsigned long long want = def.capacity ? def.capacity : 0ull + n + nnew + def.resize_plus0;
  if (want < 0ull + n + nnew) throw SphError(SPH_ERR_ARG, "the inout capacity is below the initial particles");
  if (want >= (1ull << 31)) throw SphError(SPH_ERR_ARG, "The number of particles is too big.");
  // inout cases take the full sort at every divide, as the reference does with new particles
  // appended behind np; the update's fused classification goes with the incremental divide
  inc_ok_ = false;
  inc_valid_ = false;
  inout_ = true;
  ioh_ = io;
  Grow(n, unsigned(want));
  iodev_ = allocs_.upload(&io, 1);
  // -- the new particles behind np (cells as JSph::LoadDcellParticles; UpdatePos, :101)
  std::vector<unsigned> idp(nnew), dcell(nnew);
  std::vector<double2> nxy(nnew);
  std::vector<double> nz(nnew);
  std::vector<float4> vr(nnew, make_float4(0.f, 0.f, 0.f, 1000.f));
  for (unsigned q = 0; q < nnew; q++) {
    const double x = npos[3 * size_t(q)], y = npos[3 * size_t(q) + 1], z = npos[3 * size_t(q) + 2];
    const double dx = x - C.dom_posmin[0], dy = y - C.dom_posmin[1], dz = z - C.dom_posmin[2];
    idp[q] = casenp_ + q;  // (inside the domain: checked with the zones, before anything changed)
    nxy[q] = make_double2(x, y);
    nz[q] = z;
    dcell[q] = DcelCell(C.dom_cellcode, unsigned(dx / double(C.scell)), unsigned(dy / double(C.scell)),
                        unsigned(dz / double(C.scell)));
  }
  check_hip(hipMemcpy(cur_.code, code.data(), 2 * size_t(n), hipMemcpyHostToDevice), "upload code");
  check_hip(hipMemcpy(cur_.idp + n, idp.data(), 4 * size_t(nnew), hipMemcpyHostToDevice), "upload idp");
  check_hip(hipMemcpy(cur_.code + n, ncode.data(), 2 * size_t(nnew), hipMemcpyHostToDevice), "upload code");
  check_hip(hipMemcpy(cur_.dcell + n, dcell.data(), 4 * size_t(nnew), hipMemcpyHostToDevice), "upload dcell");
  check_hip(hipMemcpy(cur_.posxy + n, nxy.data(), 16 * size_t(nnew), hipMemcpyHostToDevice), "upload posxy");
  check_hip(hipMemcpy(cur_.posz + n, nz.data(), 8 * size_t(nnew), hipMemcpyHostToDevice), "upload posz");
  check_hip(hipMemcpy(cur_.velrhop + n, vr.data(), 16 * size_t(nnew), hipMemcpyHostToDevice), "upload velrhop");
  if (cur_.velrhopm1)
    check_hip(hipMemcpy(cur_.velrhopm1 + n, vr.data(), 16 * size_t(nnew), hipMemcpyHostToDevice), "upload velrhopm1");
  const unsigned npnew = n + nnew, idmax = casenp_ + nnew - 1u;
  check_hip(hipMemcpy(&sc_->np, &npnew, 4, hipMemcpyHostToDevice), "set np");
  check_hip(hipMemcpy(&sc_->io_idmax, &idmax, 4, hipMemcpyHostToDevice), "set IdMax");
  // -- RunCellDivide and InOutUpdatePartsData of the initial time (:123-133)
  io_pass_ = 1;
  try {
    RunCellDivide();
  } catch (...) {
    io_pass_ = 0;
    throw;
  }
  io_pass_ = 0;
  Sync();
  CheckErrors();
}

SphInOutStats SphGpuSingle::InOutStats() {
  if (!inout_) throw SphError(SPH_ERR_STATE, "the solver has no inlet/outlet zones");
  Stats();
  const DevScalars& s = *sc_host_;
  SphInOutStats r;
  std::memset(&r, 0, sizeof(r));
  r.count = s.io_count;
  r.idmax = s.io_idmax;
  r.capacity = cap_;
  r.created = s.io_created;
  r.removed = s.io_removed;
  return r;
}

}  // namespace sphx
