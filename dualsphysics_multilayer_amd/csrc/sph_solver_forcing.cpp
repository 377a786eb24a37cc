// sph_solver_forcing.cpp — SphGpuSingle: imposed accelerations and damping zones (sph_forcing.hip).
#include "sph_solver.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace sphx {

// ---- imposed accelerations and damping zones (sph_forcing.hip) -------------------------------
// The damping on the velocity the update has just written (ComputeVerlet swapped it into
// cur_.velrhop); velrhopm1 / velrhoppre and the positions stay.  The update's fused
// classification and slab count pass stage dcell, code and counts only, never a velocity, and
// a slab's migrant and ghost records are packed at the divide after this: they carry the
// damped velocity, and the fusion stays on.  (Not inside the update's turn of the turns
// measurement mode 2, UpdateTurn: there k_damping may run beside another slab's kernels, which
// changes that mode's timing only.)
void SphGpuSingle::RunDamping() {
  TimedBegin(1);
  launch_damping(stream, cap_, sc_, K, G, dampzones_, ndamp_, cur_, cur_.velrhop);
  TimedEnd(1);
}

// ComputeVelocity (JDsAccInput.cpp:238-274): v += a dt, zero at the first row.
void accinput_velocities(unsigned nrows, const double* rows, double* out) {
  double t0 = 0, vel[6] = {0, 0, 0, 0, 0, 0};
  for (unsigned r = 0; r < nrows; r++) {
    const double* row = rows + 7 * size_t(r);
    double cur[6] = {0, 0, 0, 0, 0, 0};
    if (r > 0) {
      const double dt = row[0] - t0;
      for (int k = 0; k < 6; k++) cur[k] = vel[k] + (row[1 + k] * dt);
    }
    for (int k = 0; k < 6; k++) out[6 * size_t(r) + k] = vel[k] = cur[k];
    t0 = row[0];
  }
}

void SphGpuSingle::SetAccInputs(unsigned n, const SphAccInputDef* defs, unsigned nrows, const double* rows) {
  if (nn_) throw SphError(SPH_ERR_UNSUPPORTED, "imposed accelerations with NN multiphase are not implemented");
  if (stepped_ || acc_.n)
    throw SphError(SPH_ERR_STATE, "the imposed accelerations are configured once, before the first step");
  if (!n || !defs) throw SphError(SPH_ERR_ARG, "no acceleration inputs");
  if (n > unsigned(ACC_MAXIN)) throw SphError(SPH_ERR_UNSUPPORTED, "more than 16 acceleration inputs");
  AccInSet set{};
  std::vector<double> tab;
  for (unsigned i = 0; i < n; i++) {
    const SphAccInputDef& d = defs[i];
    if (d.nrows < 2) throw SphError(SPH_ERR_ARG, "Cannot be less than two registers in variable acceleration data.");
    if (d.row0 > nrows || d.nrows > nrows - d.row0) throw SphError(SPH_ERR_ARG, "acceleration input: rows out of range");
    const unsigned tv = unsigned(CODE_MASKTYPE | CODE_MASKVALUE);
    if (d.code1 > d.code2 || (d.code2 & ~tv) || (d.code1 & unsigned(CODE_MASKTYPE)) != (d.code2 & unsigned(CODE_MASKTYPE)) ||
        (d.code1 & unsigned(CODE_MASKTYPE)) < unsigned(CODE_TYPE_FLOATING))
      throw SphError(SPH_ERR_ARG, "acceleration input: the code range must select fluid blocks or floating bodies");
    for (unsigned j = 0; j < i; j++)
      if (d.code1 <= defs[j].code2 && defs[j].code1 <= d.code2)
        throw SphError(SPH_ERR_ARG, "An input already exists for the same mk.");
    AccInDev& a = set.in[i];
    a.code1 = d.code1;
    a.code2 = d.code2;
    a.gravity = d.globalgravity ? 1 : 0;
    a.first = int(tab.size() / ACC_ROWW);
    a.n = int(d.nrows);
    a.t0 = d.timestart;
    a.t1 = d.timeend;
    for (int k = 0; k < 3; k++) a.centre[k] = double(float(d.centre[k]));  // tfloat3 acccentre (JDsAccInput.cpp:184)
    std::vector<double> vel(6 * size_t(d.nrows));
    accinput_velocities(d.nrows, rows + 7 * size_t(d.row0), vel.data());
    for (unsigned r = 0; r < d.nrows; r++) {
      const double* row = rows + 7 * size_t(d.row0 + r);
      tab.insert(tab.end(), row, row + 7);
      tab.insert(tab.end(), vel.begin() + 6 * r, vel.begin() + 6 * (r + 1));
    }
  }
  set.n = int(n);
  check_hip(hipSetDevice(device), "hipSetDevice");
  double* drows = allocs_.upload(tab.data(), tab.size());
  AccState* dstate = allocs_.alloc<AccState>(ACC_MAXIN);
  AccVals* dvals = allocs_.alloc<AccVals>(ACC_MAXIN);
  check_hip(hipMemset(dstate, 0xff, sizeof(AccState) * ACC_MAXIN), "reset acceleration tables");  // pos = -1: no lookup yet
  check_hip(hipMemset(dvals, 0, sizeof(AccVals) * ACC_MAXIN), "zero acceleration values");
  accrows_ = drows;
  accstate_ = dstate;
  accvals_ = dvals;
  acc_ = set;
}

namespace {
struct P3 { double x, y, z; };
// fgeo::Plane3Pt (FunGeo3d.cpp:52-62)
void plane3pt(P3 p1, P3 p2, P3 p3, double out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  auto ne = [](P3 a, P3 b) { return a.x != b.x || a.y != b.y || a.z != b.z; };
  if (ne(p1, p2) && ne(p1, p3) && ne(p2, p3)) {
    const P3 v1{p2.x - p1.x, p2.y - p1.y, p2.z - p1.z}, v2{p3.x - p1.x, p3.y - p1.y, p3.z - p1.z};
    const P3 v{v1.y * v2.z - v1.z * v2.y, v1.z * v2.x - v1.x * v2.z, v1.x * v2.y - v1.y * v2.x};
    out[0] = v.x;
    out[1] = v.y;
    out[2] = v.z;
    out[3] = -((v.x * p1.x) + (v.y * p1.y) + (v.z * p1.z));
  }
}
}  // namespace

// The derived values of zone `i` of the list, on the host in double and in the reference's
// order of operations (JDsDampingOp_Plane / _Box / _Cylinder::ReadXml); the device evaluates
// the same numbers.
void derive_damping(const SphDampingDef& d, unsigned i, DampZoneDev& z) {
  std::memset(&z, 0, sizeof(z));
  z.over = d.overlimit;
  z.redumax = d.redumax;
  for (int k = 0; k < 3; k++) z.factor[k] = d.factorxyz[k];
  const std::string err = "Error in configuration of damping " + std::to_string(i) + ".";
  if (d.type == SPH_DAMP_PLANE) {  // JDsDampingOp_Plane::ReadXml (JDsDamping.cpp:96-130)
    z.type = DAMP_PLANE;
    const double* lmin = d.pt[0];
    const double vec[3] = {d.pt[1][0] - lmin[0], d.pt[1][1] - lmin[1], d.pt[1][2] - lmin[2]};
    const double m = std::sqrt(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2]);
    z.dist = float(m);
    // fgeo::PlanePtVec: the unit normal (the vector itself when its length is 0)
    const double u[3] = {m ? vec[0] / m : vec[0], m ? vec[1] / m : vec[1], m ? vec[2] / m : vec[2]};
    z.plane[0] = u[0];
    z.plane[1] = u[1];
    z.plane[2] = u[2];
    z.plane[3] = -u[0] * lmin[0] - u[1] * lmin[1] - u[2] * lmin[2];
    if (d.usedomain) {  // ComputeDomPlanes (JDsDamping.cpp:58-91)
      z.usedomain = 1;
      z.zmin = d.domzmin;
      z.zmax = d.domzmax;
      double vp[4][2], angles[4] = {0, 0, 0, 0};
      for (int c = 0; c < 4; c++) {
        vp[c][0] = d.dompt[c][0];
        vp[c][1] = d.dompt[c][1];
      }
      const double TODEG = 57.29577951308232087684;  // 180/PI (TypesDef.h:28)
      for (int c = 1; c < 4; c++) {
        angles[c] = std::atan2(vp[0][1] - vp[c][1], vp[0][0] - vp[c][0]) * TODEG;
        if (angles[c] < 0) angles[c] += 360.;
      }
      for (int c = 1; c < 3; c++)
        for (int c2 = c + 1; c2 < 4; c2++)
          if (angles[c] > angles[c2]) {
            std::swap(angles[c], angles[c2]);
            std::swap(vp[c][0], vp[c2][0]);
            std::swap(vp[c][1], vp[c2][1]);
          }
      for (int c = 0; c < 4; c++) {
        const int c1 = (c + 1) & 3;
        plane3pt(P3{vp[c][0], vp[c][1], 0}, P3{vp[c1][0], vp[c1][1], 0}, P3{vp[c1][0], vp[c1][1], 1}, z.dompla[c]);
      }
    }
  } else if (d.type == SPH_DAMP_BOX) {  // JDsDampingOp_Box::ReadXml (JDsDamping.cpp:345-390)
    z.type = DAMP_BOX;
    const unsigned dirs = d.directions;
    if (!dirs || (dirs & ~unsigned(SPH_DAMPDIR_ALL)))
      throw SphError(SPH_ERR_ARG, "damping box: At least one direction must be confirured.");
    double min1[3], min2[3], max1[3], max2[3], over1[3], over2[3], size1[3], size2[3];
    for (int k = 0; k < 3; k++) {
      min1[k] = d.pt[0][k];
      min2[k] = d.pt[1][k];
      max1[k] = d.pt[2][k];
      max2[k] = d.pt[3][k];
    }
    auto le = [](const double* a, const double* b) { return a[0] <= b[0] && a[1] <= b[1] && a[2] <= b[2]; };
    if (!le(min1, min2)) throw SphError(SPH_ERR_ARG, err + " Begin of LimitMin is higher than end of LimitMin.");
    if (!le(max1, max2)) throw SphError(SPH_ERR_ARG, err + " Begin of LimitMax is higher than end of LimitMax.");
    if (!le(max1, min1)) throw SphError(SPH_ERR_ARG, err + " LimitMin box is not inside of LimitMax box.");
    if (!le(min2, max2)) throw SphError(SPH_ERR_ARG, err + " LimitMin box is not inside of LimitMax box.");
    if (d.overlimit < 0) throw SphError(SPH_ERR_ARG, err + " OverLimit must be higher than 1.");
    for (int k = 0; k < 3; k++) {
      over1[k] = max1[k] - double(d.overlimit);
      over2[k] = max2[k] + double(d.overlimit);
    }
    // x: left / right, y: front / back, z: bottom / top
    const unsigned lo[3] = {SPH_DAMPDIR_LEFT, SPH_DAMPDIR_FRONT, SPH_DAMPDIR_BOTTOM};
    const unsigned hi[3] = {SPH_DAMPDIR_RIGHT, SPH_DAMPDIR_BACK, SPH_DAMPDIR_TOP};
    for (int k = 0; k < 3; k++) {
      if (!(dirs & hi[k])) max2[k] = over2[k] = min2[k];
      if (!(dirs & lo[k])) max1[k] = over1[k] = min1[k];
    }
    for (int k = 0; k < 3; k++) {
      size1[k] = min1[k] - max1[k];
      size2[k] = max2[k] - min2[k];
      if (!(dirs & hi[k]) || size2[k] < 0) size2[k] = 0;
      if (!(dirs & lo[k]) || size1[k] < 0) size1[k] = 0;
    }
    for (int k = 0; k < 3; k++) {
      z.bmin1[k] = min1[k];
      z.bmin2[k] = min2[k];
      z.bmax1[k] = max1[k];
      z.bmax2[k] = max2[k];
      z.bover1[k] = over1[k];
      z.bover2[k] = over2[k];
      z.bsize1[k] = size1[k];
      z.bsize2[k] = size2[k];
    }
  } else if (d.type == SPH_DAMP_CYLINDER) {  // JDsDampingOp_Cylinder (JDsDamping.cpp:526-542,576-577)
    z.type = DAMP_CYL;
    if (d.radmin > d.radmax) throw SphError(SPH_ERR_ARG, err + " LimitMin radius is higher than LimitMax radius.");
    for (int k = 0; k < 3; k++) {
      z.p1[k] = d.pt[0][k];
      z.p2[k] = d.pt[1][k];
    }
    z.rmin = d.radmin;
    z.dist = float(d.radmax - d.radmin);
    z.vertical = (z.p1[0] == z.p2[0] && z.p1[1] == z.p2[1]) ? 1 : 0;
    const double v[3] = {z.p1[0] - z.p2[0], z.p1[1] - z.p2[1], z.p1[2] - z.p2[2]};
    z.axislen = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  } else {
    throw SphError(SPH_ERR_ARG, "damping zone type is invalid");
  }
}

void SphGpuSingle::SetDamping(unsigned n, const SphDampingDef* defs) {
  if (nn_) throw SphError(SPH_ERR_UNSUPPORTED, "damping zones with NN multiphase are not implemented");
  if (stepped_ || ndamp_) throw SphError(SPH_ERR_STATE, "the damping zones are configured once, before the first step");
  if (!n || !defs) throw SphError(SPH_ERR_ARG, "no damping zones");
  if (n > unsigned(DAMP_MAXZONES)) throw SphError(SPH_ERR_UNSUPPORTED, "more than 16 damping zones");
  std::vector<DampZoneDev> zs(n);
  for (unsigned i = 0; i < n; i++) derive_damping(defs[i], i, zs[i]);
  check_hip(hipSetDevice(device), "hipSetDevice");
  dampzones_ = allocs_.upload(zs.data(), zs.size());
  ndamp_ = int(n);
}

}  // namespace sphx
