// sph_dem.hip — DEM collisions of floating bodies on gfx950 (RigidAlgorithm=2, the SPH-DCDEM
// coupling of Canelas et al.): JSphCpu::InteractionForcesDEM (JSphCpu.cpp:828-925), run inside
// Interaction_Forces right after the pair sums (JSphCpu.cpp:975).
//
// Reference semantics (the parity contract).  For every floating particle p1: every particle
// p2 of the bound cells, then of the fluid cells, of p1's neighbour cells (+-1 full cells, +-2
// half cells; z, y, x ascending) that is not fluid and belongs to another block is a
// candidate.  Every candidate gives demvisc (no distance cut); a candidate closer than Dp is a
// contact: Hertz stiffness (Lemieux), Cummins damping, Coulomb friction capped by the elastic
// spring over DemDtForce.  Only a p1 whose summed contact acceleration is non-zero adds it to
// ace and folds the maximum demvisc of ALL its candidates into ViscDt (JSphCpu.cpp:914-918).
//
// Work decomposition.  One lane per particle of [npb, np) in cell-sorted order, so the lanes of
// a wave that hold floating particles walk the same cell rows; a lane of a fluid particle only
// takes part in the AceMax reduction.  The walk reads p2's code first (2 B) and position and
// velocity only for a candidate; the force terms run under overlap only.  The two powf of
// demvisc are evaluated in a second walk, by the lanes whose contact sum came out non-zero:
// the rare case, and the same maximum as the reference's (a maximum has no order).  Contacts
// are summed in the reference's order, in its float operations (no contraction: the terms
// cancel, rep - gn*..., Dp - rad).  No host synchronisation; LDS: the block reductions' 16 B.
//
// AceMax: a contact can lower |ace| of the particle that held the pair-sum maximum, so the
// solver clears the AceMax slots and this kernel reduces the final |ace|^2 of [npb, np), as
// k_accinput does for imposed accelerations.
#include "sph_kernels.hpp"

namespace sphx {

struct DemP1 {
  double x, y, z;
  float vx, vy, vz;
  DemRec d;
  unsigned tav;
};

// One candidate p2: demvisc (VISC) or the contact force terms (JSphCpu.cpp:866-909).
template <bool VISC>
__device__ __forceinline__ void dem_pair(const DemP1& p, bool boundcells, float dpf, float dtforce,
                                         const DemRec* __restrict__ dem, unsigned tav2, double x2, double y2,
                                         double z2, const float4 vr2, float& ax, float& ay, float& az,
                                         float& demdt) {
#pragma clang fp contract(off)
  const float drx = float(p.x - x2), dry = float(p.y - y2), drz = float(p.z - z2);
  const float rr2 = drx * drx + dry * dry + drz * drz;
  const float rad = sqrtf(rr2);
  const float over_lap = 1.0f * dpf - rad;
  if (!VISC && !(over_lap > 0.0f)) return;
  const float masstotp2 = dem[tav2].mass, taup2 = dem[tav2].tau;
  const float nu_mass = (boundcells ? p.d.mass / 2 : p.d.mass * masstotp2 / (p.d.mass + masstotp2));
  const float kn = 4 / (3 * (p.d.tau + taup2)) * sqrtf(dpf / 4);
  const float dvx = p.vx - vr2.x, dvy = p.vy - vr2.y, dvz = p.vz - vr2.z;
  const float nx = drx / rad, ny = dry / rad, nz = drz / rad;
  const float vn = dvx * nx + dvy * ny + dvz * nz;
  if (VISC) {
    const float demvisc = 0.2f / (3.21f * (powf(nu_mass / kn, 0.4f) * powf(fabsf(vn), -0.2f)) / 40.f);
    if (demdt < demvisc) demdt = demvisc;
    return;
  }
  const float kfricp2 = dem[tav2].kfric, restitup2 = dem[tav2].restitu;
  // normal
  const float eij = (p.d.restitu + restitup2) / 2;
  const float leij = logf(eij);
  const float gn = -(2.0f * leij * sqrtf(nu_mass * kn)) / (sqrtf(3.14159265358979323846f + leij * leij));
  const float rep = kn * powf(over_lap, 1.5f);
  const float fn = rep - gn * powf(over_lap, 0.25f) * vn;
  float acef = fn / p.d.massp;
  ax += (acef * nx);
  ay += (acef * ny);
  az += (acef * nz);
  // tangential
  const float dvxt = dvx - vn * nx, dvyt = dvy - vn * ny, dvzt = dvz - vn * nz;
  const float vt = sqrtf(dvxt * dvxt + dvyt * dvyt + dvzt * dvzt);
  float tx = 0, ty = 0, tz = 0;
  if (vt != 0) {
    tx = dvxt / vt;
    ty = dvyt / vt;
    tz = dvzt / vt;
  }
  const float ft_elast = 2 * (kn * dtforce - gn) * vt / 7;
  const float kfric_ij = (p.d.kfric + kfricp2) / 2;
  float ft = kfric_ij * fn * tanhf(8 * vt);
  ft = (ft < ft_elast ? ft : ft_elast);
  acef = ft / p.d.massp;
  ax += (acef * tx);
  ay += (acef * ty);
  az += (acef * tz);
}

// The candidates of p1 in the reference's order: bound cells, then fluid cells; z, y, x ascending.
template <bool VISC>
__device__ __forceinline__ void dem_walk(const DemP1& p, int cx, int cy, int cz, const DivGrid& g, int sd,
                                         float dpf, float dtforce, const DemRec* __restrict__ dem,
                                         const unsigned* __restrict__ begincell, const PartArrays& a, float& ax,
                                         float& ay, float& az, float& demdt) {
  const int xi = max(cx - sd, 0), xf = min(cx + sd, g.ncx - 1) + 1;
  const int yi = max(cy - sd, 0), yf = min(cy + sd, g.ncy - 1) + 1;
  const int zi = max(cz - sd, 0), zf = min(cz + sd, g.ncz - 1) + 1;
  for (int tpfluid = 0; tpfluid <= 1; tpfluid++) {
    const unsigned cellinit = tpfluid ? g.boxfluid : 0u;
    for (int z = zi; z < zf; z++)
      for (int y = yi; y < yf; y++) {
        const unsigned row = cellinit + unsigned(z) * g.nsheet + unsigned(y) * unsigned(g.ncx);
        const unsigned pini = begincell[row + xi], pfin = begincell[row + xf];  // the row's cells are contiguous
        for (unsigned p2 = pini; p2 < pfin; p2++) {
          const typecode c2 = a.code[p2];
          const unsigned tav2 = unsigned(c2) & unsigned(CODE_MASKTYPE | CODE_MASKVALUE);
          if (CodeIsFluid(c2) || tav2 == p.tav) continue;
          const double2 pxy = a.posxy[p2];
          dem_pair<VISC>(p, !tpfluid, dpf, dtforce, dem, tav2, pxy.x, pxy.y, a.posz[p2], a.velrhop[p2], ax, ay, az,
                         demdt);
        }
      }
  }
}

__global__ __launch_bounds__(256) void k_dem(DevScalars* __restrict__ sc, KConst K, DivGrid g, float dpf,
                                             const DemRec* __restrict__ dem,
                                             const unsigned* __restrict__ begincell, PartArrays a, int interstep,
                                             float4* __restrict__ arace) {
  const unsigned np = sc->np, npb = sc->npb;
  const unsigned p1 = npb + blockIdx.x * blockDim.x + threadIdx.x;
  float ace2 = 0.f, demdt = 0.f;
  if (p1 < np) {
    float4 ra = arace[p1];
    const typecode c1 = a.code[p1];
    if (CodeType(c1) == CODE_TYPE_FLOATING) {
      // DemDtForce of this interaction (JSphCpuSingle.cpp:678,700,709)
      const float dtforce = float(interstep == 1 ? sc->demdtforce : interstep == 2 ? sc->symdtpre * 0.5 : sc->dt);
      DemP1 p;
      const double2 pxy = a.posxy[p1];
      const float4 vr1 = a.velrhop[p1];
      p.x = pxy.x;
      p.y = pxy.y;
      p.z = a.posz[p1];
      p.vx = vr1.x;
      p.vy = vr1.y;
      p.vz = vr1.z;
      p.tav = unsigned(c1) & unsigned(CODE_MASKTYPE | CODE_MASKVALUE);
      p.d = dem[p.tav];
      const unsigned dc = a.dcell[p1];
      const int cx = int(DcelCellx(K.domcellcode, dc)), cy = int(DcelCelly(K.domcellcode, dc)),
                cz = int(DcelCellz(K.domcellcode, dc));
      float ax = 0.f, ay = 0.f, az = 0.f, unused = 0.f;
      dem_walk<false>(p, cx, cy, cz, g, K.scelldiv, dpf, dtforce, dem, begincell, a, ax, ay, az, unused);
      if (ax != 0.f || ay != 0.f || az != 0.f) {
        dem_walk<true>(p, cx, cy, cz, g, K.scelldiv, dpf, dtforce, dem, begincell, a, ax, ay, az, demdt);
        ra.x += ax;
        if (!K.sim2d) ra.y += ay;  // Simulate2D: Acec[].y = 0 after the interaction (JSphCpuSingle.cpp:544-549)
        ra.z += az;
        arace[p1] = ra;
      }
    }
    ace2 = ra.x * ra.x + ra.y * ra.y + ra.z * ra.z;
  }
  block_max_atomic(sc, RED_VISCDT, demdt);
  __syncthreads();  // the two reductions share the block's four LDS words
  block_max_atomic(sc, RED_ACEMAX2, ace2);
}

void launch_dem(hipStream_t stm, unsigned cap, DevScalars* sc, const KConst& K, const DivGrid& g, float dp,
                const DemRec* dem, const unsigned* begincell, const PartArrays& a, int interstep, float4* arace) {
  hipLaunchKernelGGL(k_dem, dim3((cap + 255) / 256), dim3(256), 0, stm, sc, K, g, dp, dem, begincell, a, interstep,
                     arace);
}

}  // namespace sphx
