// sph_forcing.hip — imposed accelerations and damping zones on CDNA4.
//
// k_accinput: JDsAccInput::RunCpu (JDsAccInput.cpp:341-393).  The reference adds the imposed
// acceleration to the zeroed Acec before the pair interaction (JSphCpu.cpp:444); here the pair
// sums are in arace already and the imposed part, formed in double from a zero base and rounded
// to float as there, is added onto them.  AceMax (JSphCpuSingle.cpp:564) is taken over the final
// Acec: the interaction kernels' maximum of the pair sums alone is no bound of it, so the solver
// resets those slots and this kernel reduces |ace|^2 of every particle of [npb, np) again.
// k_damping: JDsDamping::ComputeDampingCpu (JDsDamping.cpp:185-232, 448-493, 573-611), every
// zone in list order on one particle, after the last update of the step.
// Both are one thread per particle; the loops over the inputs / zones are wave-uniform.
#include <cfloat>

#include "sph_forcing.hpp"

namespace sphx {

// JLinearValue::FindTime + GetValue3d3d (JLinearValue.cpp:209-247, 344-382) of the two
// 6-value tables of one input (rows of ACC_ROWW doubles): the walk continues from the row of
// the last call, and a call at the TimeStep of the last one keeps its interval (the Symplectic
// predictor and corrector of one step), as sph_bodies.hip restates it for the floating tables.
__device__ void acc_table_eval(const double* __restrict__ rows, const AccInDev& in, AccState& d, double t, AccVals& o) {
  const double* T = rows + size_t(in.first) * ACC_ROWW;
  const int n = in.n;
  if (d.pos < 0 || t != d.t) {
    int pos = d.pos < 0 ? 0 : d.pos, posnext = pos;
    double tpre = T[pos * ACC_ROWW], tnext = tpre;
    if (n > 1) {
      while (tpre >= t && pos > 0) tpre = T[--pos * ACC_ROWW];  // back
      posnext = pos + 1 < n ? pos + 1 : pos;
      tnext = T[posnext * ACC_ROWW];
      while (tnext < t && posnext + 1 < n) tnext = T[++posnext * ACC_ROWW];  // forward
      if (posnext - pos > 1) pos = posnext - 1;
    }
    d.pos = pos;
    d.posnext = posnext;
    d.t = t;
  }
  const double* A = T + d.pos * ACC_ROWW;
  const double* B = T + d.posnext * ACC_ROWW;
  const double tdif = B[0] - A[0];
  double f = tdif != 0.0 ? (t - A[0]) / tdif : 0.0;
  if (f < 0.) f = 0.;
  if (f > 1.) f = 1.;
  double v[12];
  for (int k = 0; k < 12; k++) {
    if (f == 0.) v[k] = A[1 + k];
    else if (f >= 1.) v[k] = B[1 + k];
    else v[k] = __dadd_rn(__dmul_rn(__dsub_rn(B[1 + k], A[1 + k]), f), A[1 + k]);
  }
  for (int k = 0; k < 3; k++) {
    o.acclin[k] = v[k];
    o.accang[k] = v[3 + k];
    o.vellin[k] = v[6 + k];
    o.velang[k] = v[9 + k];
  }
  o.withang = (o.accang[0] != 0 || o.accang[1] != 0 || o.accang[2] != 0) ? 1 : 0;
}

// JDsAccInputMk::GetAccValues (JDsAccInput.cpp:99-113) of every input at the interaction's
// TimeStep, held on the device: the corrector's interaction runs after k_dt advanced the time,
// at the step's start (tstep0) as the reference's.
__global__ void k_accinput_eval(const DevScalars* __restrict__ sc, AccInSet set, const double* __restrict__ rows,
                                AccState* __restrict__ state, AccVals* __restrict__ vals, int interstep) {
  const int i = threadIdx.x;
  if (i >= set.n) return;
  const double t = (interstep == 3 ? sc->tstep0 : sc->time);
  const AccInDev& in = set.in[i];
  AccVals o;
  o.active = 0;
  o.withang = 0;
  for (int k = 0; k < 3; k++) o.acclin[k] = o.accang[k] = o.vellin[k] = o.velang[k] = 0.;
  if (in.t0 <= t && t <= in.t1) {
    AccState d = state[i];
    acc_table_eval(rows, in, d, t, o);
    state[i] = d;
    o.active = 1;
  }
  vals[i] = o;
}

__global__ __launch_bounds__(256) void k_accinput(DevScalars* __restrict__ sc, KConst K, DivGrid g, AccInSet set,
                                                  const AccVals* __restrict__ vals, PartArrays a,
                                                  float4* __restrict__ arace) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned np = sc->np, npb = sc->npb;
  float ace2 = 0.f;
  bool own = (p >= npb && p < np);
  if (own && g.split()) own = slab_owned(g, slab_local(g, K.domcellcode, a.dcell[p]));  // a ghost's owner adds it
  if (own) {
    float4 ra = arace[p];
    const unsigned tav = unsigned(a.code[p]) & unsigned(CODE_MASKTYPE | CODE_MASKVALUE);
    for (int c = 0; c < set.n; c++) {
      const AccInDev& in = set.in[c];
      if (!vals[c].active || tav < in.code1 || tav > in.code2) continue;
      const AccVals& v = vals[c];
      double ax = 0. + v.acclin[0], ay = 0. + v.acclin[1], az = 0. + v.acclin[2];
      if (!in.gravity) {
        ax -= double(K.gravx);
        ay -= double(K.gravy);
        az -= double(K.gravz);
      }
      if (v.withang) {
        const double2 pxy = a.posxy[p];
        const float4 vr = a.velrhop[p];
        const double dcx = pxy.x - in.centre[0], dcy = pxy.y - in.centre[1], dcz = a.posz[p] - in.centre[2];
        const double vx = double(vr.x), vy = double(vr.y), vz = double(vr.z);
        // (Dw/Dt) x (r_i - r)
        ax += nc(v.accang[1] * dcz) - nc(v.accang[2] * dcy);
        ay += nc(v.accang[2] * dcx) - nc(v.accang[0] * dcz);
        az += nc(v.accang[0] * dcy) - nc(v.accang[1] * dcx);
        // w x (w x (r_i - r))
        const double inx = nc(v.velang[1] * dcz) - nc(v.velang[2] * dcy);
        const double iny = nc(v.velang[2] * dcx) - nc(v.velang[0] * dcz);
        const double inz = nc(v.velang[0] * dcy) - nc(v.velang[1] * dcx);
        ax += nc(v.velang[1] * inz) - nc(v.velang[2] * iny);
        ay += nc(v.velang[2] * inx) - nc(v.velang[0] * inz);
        az += nc(v.velang[0] * iny) - nc(v.velang[1] * inx);
        // Coriolis term, component by component as JDsAccInput.cpp:383-385 writes it
        ax += nc((2.0 * v.velang[1]) * vz) - nc((2.0 * v.velang[2]) * (vy - v.vellin[1]));
        ay += nc((2.0 * v.velang[2]) * vx) - nc((2.0 * v.velang[0]) * (vz - v.vellin[2]));
        az += nc((2.0 * v.velang[0]) * vy) - nc((2.0 * v.velang[1]) * (vx - v.vellin[0]));
      }
      ra.x += float(ax);
      if (!K.sim2d) ra.y += float(ay);  // Simulate2D: Acec[].y = 0 after the interaction
      ra.z += float(az);
      arace[p] = ra;
      break;  // the ranges are disjoint (the reference refuses an mk configured twice)
    }
    ace2 = ra.x * ra.x + ra.y * ra.y + ra.z * ra.z;
  }
  block_max_atomic(sc, RED_ACEMAX2, ace2);
}

void launch_accinput(hipStream_t stm, unsigned cap, DevScalars* sc, const KConst& K, const DivGrid& g,
                     const AccInSet& set, const double* rows, AccState* state, AccVals* vals, int interstep,
                     const PartArrays& a, float4* arace) {
  hipLaunchKernelGGL(k_accinput_eval, dim3(1), dim3(64), 0, stm, sc, set, rows, state, vals, interstep);
  hipLaunchKernelGGL(k_accinput, dim3((cap + 255) / 256), dim3(256), 0, stm, sc, K, g, set, vals, a, arace);
}

// fdis^2 -> the three velocity factors max(0, 1 - dt fdis^2 redumax factorxyz), applied as
// float(double factor * vel).
__device__ __forceinline__ void damp_apply(const DampZoneDev& z, double dt, double fdis, float4& v) {
  const double redudt = nc(nc(dt * nc(fdis * fdis)) * double(z.redumax));
  double rx = 1. - nc(redudt * double(z.factor[0]));
  double ry = 1. - nc(redudt * double(z.factor[1]));
  double rz = 1. - nc(redudt * double(z.factor[2]));
  rx = (rx < 0 ? 0. : rx);
  ry = (ry < 0 ? 0. : ry);
  rz = (rz < 0 ? 0. : rz);
  v.x = float(rx * double(v.x));
  v.y = float(ry * double(v.y));
  v.z = float(rz * double(v.z));
}
__device__ __forceinline__ double plane_point(const double pl[4], double x, double y, double z) {
  return nc(pl[0] * x) + nc(pl[1] * y) + nc(pl[2] * z) + pl[3];
}
__device__ __forceinline__ bool le3(const double a[3], double x, double y, double z) {
  return a[0] <= x && a[1] <= y && a[2] <= z;
}
__device__ __forceinline__ bool ge3(const double a[3], double x, double y, double z) {
  return x <= a[0] && y <= a[1] && z <= a[2];
}

__global__ __launch_bounds__(256) void k_damping(const DevScalars* __restrict__ sc, KConst K, DivGrid g,
                                                 const DampZoneDev* __restrict__ zones, int nzones, PartArrays a,
                                                 float4* __restrict__ velrhop) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= sc->np || p < sc->npb || halted(sc)) return;
  const typecode code = a.code[p];
  if (!(CodeIsNormal(code) && CodeIsFluid(code))) return;  // no floating, no excluded particles
  // A slab's ghosts are damped by their owner.  The update has already written the NEW dcell: an
  // owned particle that has just crossed the face holds a cell of the neighbour's columns and is
  // still this slab's to damp (it migrates at the divide, with the damped velocity); the ghosts
  // are the ones the update marked (as k_move_bound tells them).
  if (g.split() && a.dcell[p] == DCELL_DISCARD) return;
  const double2 pxy = a.posxy[p];
  const double x = pxy.x, y = pxy.y, z = a.posz[p];
  const float4 v0 = velrhop[p];
  float4 v = v0;
  const double dt = sc->dt;
  for (int c = 0; c < nzones; c++) {
    const DampZoneDev& zn = zones[c];
    if (zn.type == DAMP_PLANE) {
      const double vdis = plane_point(zn.plane, x, y, z);
      if (!(0 < vdis && vdis <= double(zn.dist + zn.over))) continue;
      if (zn.usedomain && !(z >= zn.zmin && z <= zn.zmax && plane_point(zn.dompla[0], x, y, z) <= 0 &&
                            plane_point(zn.dompla[1], x, y, z) <= 0 && plane_point(zn.dompla[2], x, y, z) <= 0 &&
                            plane_point(zn.dompla[3], x, y, z) <= 0))
        continue;
      damp_apply(zn, dt, vdis >= double(zn.dist) ? 1. : vdis / double(zn.dist), v);
    } else if (zn.type == DAMP_BOX) {
      if (!(le3(zn.bover1, x, y, z) && ge3(zn.bover2, x, y, z))) continue;  // outside the overlimit domain
      if (le3(zn.bmin1, x, y, z) && ge3(zn.bmin2, x, y, z)) continue;       // inside the free domain
      double fdis = 1.;
      if (le3(zn.bmax1, x, y, z) && ge3(zn.bmax2, x, y, z)) {
        fdis = 0;
        double s;
        if (zn.bsize2[2]) { s = (z - zn.bmin2[2]) / zn.bsize2[2]; fdis = (fdis >= s ? fdis : s); }
        if (zn.bsize2[1]) { s = (y - zn.bmin2[1]) / zn.bsize2[1]; fdis = (fdis >= s ? fdis : s); }
        if (zn.bsize2[0]) { s = (x - zn.bmin2[0]) / zn.bsize2[0]; fdis = (fdis >= s ? fdis : s); }
        if (zn.bsize1[2]) { s = (zn.bmin1[2] - z) / zn.bsize1[2]; fdis = (fdis >= s ? fdis : s); }
        if (zn.bsize1[1]) { s = (zn.bmin1[1] - y) / zn.bsize1[1]; fdis = (fdis >= s ? fdis : s); }
        if (zn.bsize1[0]) { s = (zn.bmin1[0] - x) / zn.bsize1[0]; fdis = (fdis >= s ? fdis : s); }
      }
      damp_apply(zn, dt, fdis, v);
    } else {
      double r;
      if (zn.vertical) {
        const double dx = x - zn.p1[0], dy = y - zn.p1[1];
        r = sqrt(nc(dx * dx) + nc(dy * dy));
      } else {  // fgeo::LinePointDist: 2 TriangleArea(pt, p1, p2) / |p1 p2| (FunGeo3d.cpp:229-246)
        const double qx = zn.p1[0] - x, qy = zn.p1[1] - y, qz = zn.p1[2] - z;
        const double rx = zn.p2[0] - x, ry = zn.p2[1] - y, rz = zn.p2[2] - z;
        const double vi = nc(qy * rz) - nc(ry * qz), vj = -(nc(qx * rz) - nc(rx * qz)), vk = nc(qx * ry) - nc(rx * qy);
        const double ar = .5 * sqrt(nc(vi * vi) + nc(vj * vj) + nc(vk * vk));
        r = (ar * 2) / zn.axislen;
      }
      const double vdis = r - zn.rmin;
      if (!(0 < vdis && vdis <= double(zn.dist + zn.over))) continue;
      damp_apply(zn, dt, vdis >= double(zn.dist) ? 1. : vdis / double(zn.dist), v);
    }
  }
  if (v.x != v0.x || v.y != v0.y || v.z != v0.z) velrhop[p] = v;
}

void launch_damping(hipStream_t stm, unsigned cap, const DevScalars* sc, const KConst& K, const DivGrid& g,
                    const DampZoneDev* zones, int nzones, const PartArrays& a, float4* velrhop) {
  hipLaunchKernelGGL(k_damping, dim3((cap + 255) / 256), dim3(256), 0, stm, sc, K, g, zones, nzones, a, velrhop);
}

}  // namespace sphx
