// sph_gauge.hip — gauge kernels (JDsGaugeItem.cpp; the reference's JDsGauge_ker.cu gives a
// velocity gauge one lane, every SWL point one serial lane and MaxZ one thread).
//
// k_gauge_eval: one wave64 per sample point (a velocity gauge has one, an SWL gauge PointNp+1,
// a MaxZ gauge one wave for its whole cell box).  A wave whose gauge is not due at sc->time
// returns at once.  Its lanes stride over the candidates of the (2 scelldiv + 1)^2 cell rows of
// the point; a row is one contiguous range begincell[v + cxini] .. begincell[v + cxfin] of the
// fluid half of the cell table (nsearch::Init / ParticleRange, JCellSearch_inline.h:54-80).  Pair
// terms are formed in float as the reference forms them, accumulated per lane in double and
// reduced over the wave by a fixed butterfly, so two runs give the same bits.
// k_gauge_force: GF_LANES lanes per boundary particle p < npbok of the target block, per-block
// sums in double (fixed order).
// k_gauge_commit: one block after them; finishes the results (the SWL scan, the force fold),
// updates the schedules and appends the records in gauge order.  No kernel communicates
// between workgroups inside a launch, and none writes anything the solver reads.
#include "sph_gauge.hpp"

namespace sphx {
namespace {

constexpr int GB = 256;  // threads per block (4 waves)
constexpr int GW = GB / 64;
// Force gauge: lanes that share one boundary particle (they stride over the candidates of its
// rows).  With one lane per particle the kernel is a chain of ~1000 dependent candidate
// visits per wet wall particle on the few waves that hold wet particles (328 us on the 1M dam
// break); 8 lanes shorten the chain and put 8x the waves in flight.
constexpr int GF_LANES = 8;
constexpr int GF_PART = GB / GF_LANES;  // boundary particles per block

__device__ __forceinline__ double wsum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wmax_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// nsearch::Init(pos, false, dvd) (JCellSearch_inline.h:54-69); false when the position has no
// cell in the domain (the reference reads out of range there).
struct NgBox {
  int cxini, cxfin, yini, yfin, zini, zfin;
};
__device__ __forceinline__ bool ng_init(double px, double py, double pz, const KConst& K, const DivGrid& g, NgBox& b) {
  const int cx = cell_of(px - K.map_realposmin_x, K.scelld), cy = cell_of(py - K.map_realposmin_y, K.scelld),
            cz = cell_of(pz - K.map_realposmin_z, K.scelld);
  if (cx < 0 || cy < 0 || cz < 0 || cx >= g.ncx || cy >= g.ncy || cz >= g.ncz) return false;
  const int s = K.scelldiv;
  b.cxini = cx - min(cx, s);
  b.cxfin = cx + min(g.ncx - cx - 1, s) + 1;
  b.yini = cy - min(cy, s);
  b.yfin = cy + min(g.ncy - cy - 1, s) + 1;
  b.zini = cz - min(cz, s);
  b.zfin = cz + min(g.ncz - cz - 1, s) + 1;
  return true;
}

// JGaugeItem::PointIsOut (JDsGaugeItem.h:125).
__device__ __forceinline__ bool point_is_out(double px, double py, double pz, const KConst& K) {
  return px != px || py != py || pz != pz || px < K.map_realposmin_x || py < K.map_realposmin_y ||
         pz < K.map_realposmin_z || px >= K.map_realposmin_x + K.map_realsize_x ||
         py >= K.map_realposmin_y + K.map_realsize_y || pz >= K.map_realposmin_z + K.map_realsize_z;
}

// GetKernelWendland_Wab / _Fac (FunSphKernel.h:206-222).
__device__ __forceinline__ float wendland_wab(const KConst& K, float rr2) {
  const float rad = sqrtf(rr2);
  const float qq = rad / K.kernelh;
  const float wqq = qq + qq + 1.f;
  const float wqq1 = 1.f - 0.5f * qq;
  const float wqq2 = wqq1 * wqq1;
  return K.awen * wqq * wqq2 * wqq2;
}
__device__ __forceinline__ float wendland_fac(const KConst& K, float rr2) {
  const float rad = sqrtf(rr2);
  const float qq = rad / K.kernelh;
  const float wqq1 = 1.f - 0.5f * qq;
  return K.bwen * qq * wqq1 * wqq1 * wqq1 / rad;
}

// fsph::ComputePress (FunSphEos.h:38-40): b (pow(rho / rho0, gamma) - 1) in float, the power
// rounded once from double (an integer gamma by exact squaring, as the divide's EOS).
__device__ __forceinline__ float gauge_press(const KConst& K, int ig, float rho) {
  const double x = double(rho / K.rhopzero);
  double xg;
  if (ig > 0) {
    double r = 1.0, b = x;
    for (int e = ig; e; e >>= 1) {
      if (e & 1) r *= b;
      b *= b;
    }
    xg = r;
  } else {
    xg = pow(x, double(K.gamma));
  }
  return K.cteb * (float(xg) - 1.0f);
}
__device__ __forceinline__ int integer_gamma(const KConst& K) {
  return (K.gamma == float(int(K.gamma)) && K.gamma >= 1.f && K.gamma <= 16.f) ? int(K.gamma) : 0;
}

__global__ __launch_bounds__(GB) void k_gauge_eval(GaugeSet gs, const DevScalars* __restrict__ sc, PartArrays a,
                                                   const unsigned* __restrict__ bc, DivGrid g, KConst K, int all) {
  if (!all && halted(sc)) return;
  const unsigned w = blockIdx.x * GW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= gs.npts) return;
  const GaugePoint pt = gs.pts[w];
  const GaugeDev& gd = gs.gauges[pt.gauge];
  if (!all && !gauge_update(gd.s, sc->time)) return;
  const int type = gd.type;
  if (type == GAUGE_MAXZ) {
    // JGaugeMaxZ::CalculeCpu (JDsGaugeItem.cpp:780-821): cell layers from the top down, the
    // highest qualifying fluid particle of the first layer that holds one
    const double scell = K.scelld;
    const int cx = cell_of(pt.x - K.map_realposmin_x, scell), cy = cell_of(pt.y - K.map_realposmin_y, scell),
              cz = cell_of(pt.z - K.map_realposmin_z, scell), cz2 = cell_of(pt.z + gd.height - K.map_realposmin_z, scell);
    const int ncel = int(fminf(ceilf(gd.distlimit / K.scell), 1.0e6f));  // (bounded: the box is clipped to the grid)
    const int cxini = max(cx - ncel, 0), cxfin = min(cx + ncel + 1, g.ncx);
    const int yini = max(cy - ncel, 0), yfin = min(cy + ncel + 1, g.ncy);
    const int zini = max(cz - ncel, 0), zfin = min(cz2 + ncel + 1, g.ncz);
    const float maxdist2 = gd.distlimit * gd.distlimit;
    const double none = -1.7976931348623157e308;
    double zmax = none;
    if (cxini < cxfin) {
      for (int z = zfin - 1; z >= zini && zmax == none; z--) {
        double best = none;
        for (int y = yini; y < yfin; y++) {
          const unsigned v = g.boxfluid + g.nsheet * unsigned(z) + unsigned(g.ncx) * unsigned(y);
          const unsigned pini = bc[v + unsigned(cxini)], pfin = bc[v + unsigned(cxfin)];
          for (unsigned p2 = pini + lane; p2 < pfin; p2 += 64) {
            const double2 pxy = a.posxy[p2];
            const float drx = float(pt.x - pxy.x), dry = float(pt.y - pxy.y);
            const float rr2 = drx * drx + dry * dry;
            if (rr2 <= maxdist2 && CodeIsFluid(a.code[p2])) best = fmax(best, a.posz[p2]);
          }
        }
        zmax = wmax_d(best);
      }
    }
    if (lane == 0) gs.ptout[w] = make_double4(zmax, 0.0, 0.0, 0.0);
    return;
  }
  // JGaugeVelocity::CalculeCpuT (JDsGaugeItem.cpp:325-369) / JGaugeSwl::CalculeMassCpu (:546-570)
  double sx = 0, sy = 0, sz = 0, sm = 0;
  NgBox b;
  bool in = ng_init(pt.x, pt.y, pt.z, K, g, b);
  if (type == GAUGE_VEL && point_is_out(pt.x, pt.y, pt.z, K)) in = false;
  if (in) {
    for (int z = b.zini; z < b.zfin; z++)
      for (int y = b.yini; y < b.yfin; y++) {
        const unsigned v = g.boxfluid + g.nsheet * unsigned(z) + unsigned(g.ncx) * unsigned(y);
        const unsigned pini = bc[v + unsigned(b.cxini)], pfin = bc[v + unsigned(b.cxfin)];
        for (unsigned p2 = pini + lane; p2 < pfin; p2 += 64) {
          const double2 pxy = a.posxy[p2];
          const float drx = float(pt.x - pxy.x), dry = float(pt.y - pxy.y), drz = float(pt.z - a.posz[p2]);
          const float rr2 = drx * drx + dry * dry + drz * drz;
          if (rr2 <= K.kernelsize2 && rr2 >= ALMOSTZERO && CodeIsFluid(a.code[p2])) {
            float wab = wendland_wab(K, rr2);
            const float4 v2 = a.velrhop[p2];
            wab *= K.massfluid / v2.w;
            if (type == GAUGE_VEL) {
              sx += double(wab * v2.x);
              sy += double(wab * v2.y);
              sz += double(wab * v2.z);
            } else {
              sm += double(wab * K.massfluid);
            }
          }
        }
      }
  }
  sx = wsum_d(sx);
  sy = wsum_d(sy);
  sz = wsum_d(sz);
  sm = wsum_d(sm);
  if (lane == 0) gs.ptout[w] = make_double4(sx, sy, sz, sm);
}

// JGaugeForce::CalculeCpuT (JDsGaugeItem.cpp:986-1040): the pressure term of the momentum
// equation on every particle of the block, from the fluid only.
__global__ __launch_bounds__(GB) void k_gauge_force(GaugeSet gs, const DevScalars* __restrict__ sc, PartArrays a,
                                                    const unsigned* __restrict__ bc, DivGrid g, KConst K, int all) {
  if (!all && halted(sc)) return;
  __shared__ double red[3][GW];
  const unsigned p1 = blockIdx.x * GF_PART + threadIdx.x / GF_LANES, sub = threadIdx.x % GF_LANES;
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double t = sc->time;
  const int ig = integer_gamma(K);
  const bool live = p1 < sc->npbok;
  const typecode code1 = live ? a.code[p1] : typecode(0);
  for (unsigned f = 0; f < gs.nforce; f++) {
    const GaugeDev& gd = gs.gauges[gs.fidx[f]];
    if (!all && !gauge_update(gd.s, t)) continue;  // (uniform over the block)
    double ax = 0, ay = 0, az = 0;
    NgBox b;
    if (live && unsigned(code1 & (CODE_MASKTYPE | CODE_MASKVALUE)) == gd.code && CodeIsNormal(code1)) {
      const double2 pxy1 = a.posxy[p1];
      const double pz1 = a.posz[p1];
      if (ng_init(pxy1.x, pxy1.y, pz1, K, g, b)) {
        const float rho1 = a.velrhop[p1].w;
        const float press1 = gauge_press(K, ig, rho1);
        for (int z = b.zini; z < b.zfin; z++)
          for (int y = b.yini; y < b.yfin; y++) {
            const unsigned v = g.boxfluid + g.nsheet * unsigned(z) + unsigned(g.ncx) * unsigned(y);
            const unsigned pini = bc[v + unsigned(b.cxini)], pfin = bc[v + unsigned(b.cxfin)];
            for (unsigned p2 = pini + sub; p2 < pfin; p2 += GF_LANES) {
              const double2 pxy = a.posxy[p2];
              const float drx = float(pxy1.x - pxy.x), dry = float(pxy1.y - pxy.y), drz = float(pz1 - a.posz[p2]);
              const float rr2 = drx * drx + dry * dry + drz * drz;
              if (rr2 <= K.kernelsize2 && rr2 >= ALMOSTZERO && CodeIsFluid(a.code[p2])) {
                const float fac = wendland_fac(K, rr2);
                const float frx = fac * drx, fry = fac * dry, frz = fac * drz;
                const float rho2 = a.velrhop[p2].w;
                const float press2 = gauge_press(K, ig, rho2);
                const float prs = (press1 + press2) / (rho1 * rho2);
                const float p_vpm1 = -prs * K.massfluid;
                ax += double(p_vpm1 * frx);
                ay += double(p_vpm1 * fry);
                az += double(p_vpm1 * frz);
              }
            }
          }
      }
    }
    ax = wsum_d(ax);
    ay = wsum_d(ay);
    az = wsum_d(az);
    if (lane == 0) {
      red[0][wave] = ax;
      red[1][wave] = ay;
      red[2][wave] = az;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      double s = 0;
      for (int k = 0; k < GW; k++) s += red[threadIdx.x][k];
      gs.fpart[(size_t(f) * gs.nfblk + blockIdx.x) * 3 + threadIdx.x] = s;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(GB) void k_gauge_commit(GaugeSet gs, DevScalars* __restrict__ sc, KConst K, int record) {
  if (record && halted(sc)) return;
  __shared__ double red[GB];
  __shared__ unsigned wtot[GW];
  __shared__ unsigned nrec;
  const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double t = sc->time;
  // the force gauges: their per-block sums folded in a fixed order
  for (unsigned f = 0; f < gs.nforce; f++) {
    GaugeDev& gd = gs.gauges[gs.fidx[f]];
    if (record && !gauge_update(gd.s, t)) continue;  // (uniform)
    for (int k = 0; k < 3; k++) {
      double s = 0;
      for (unsigned b = tid; b < gs.nfblk; b += GB) s += gs.fpart[(size_t(f) * gs.nfblk + b) * 3 + k];
      red[tid] = s;
      __syncthreads();
      for (unsigned off = GB / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
      }
      if (tid == 0) gd.res[k] = float(red[0]) * K.massbound;  // acesum * MassBound
      __syncthreads();
    }
  }
  if (tid == 0) nrec = gs.ctl->count;
  __syncthreads();
  for (unsigned base = 0; base < gs.ng; base += GB) {
    const unsigned gi = base + tid;
    bool emit = false;
    float r0 = 0, r1 = 0, r2 = 0;
    if (gi < gs.ng) {
      GaugeDev& gd = gs.gauges[gi];
      GaugeSched s = gd.s;
      if (!record || gauge_update(s, t)) {
        if (gd.type == GAUGE_VEL) {
          const double4 o = gs.ptout[gd.pt0];
          r0 = float(o.x);
          r1 = float(o.y);
          r2 = float(o.z);
        } else if (gd.type == GAUGE_SWL) {
          // JGaugeSwl::CalculeCpuT (JDsGaugeItem.cpp:580-596): the first point below MassLimit
          // after a point above it
          const float ml = gd.masslimit;
          float mpre = 0;
          bool found = false;
          double px = 0, py = 0, pz = 0;
          for (unsigned cp = 0; cp <= gd.pointnp && !found; cp++) {
            const float mass = float(gs.ptout[gd.pt0 + cp].w);
            if (mass > ml) mpre = mass;
            if (mass < ml && mpre) {
              const float fxm1 = (ml - mpre) / (mass - mpre) - 1;
              const GaugePoint q = gs.pts[gd.pt0 + cp];
              px = q.x + gd.dir[0] * double(fxm1);
              py = q.y + gd.dir[1] * double(fxm1);
              pz = q.z + gd.dir[2] * double(fxm1);
              found = true;
            }
          }
          if (!found) {
            const double m = mpre ? double(gd.pointnp) : 0.0;
            px = gd.p0[0] + gd.dir[0] * m;
            py = gd.p0[1] + gd.dir[1] * m;
            pz = gd.p0[2] + gd.dir[2] * m;
          }
          r0 = float(px);
          r1 = float(py);
          r2 = float(pz);
        } else if (gd.type == GAUGE_MAXZ) {
          r0 = fmaxf(float(gs.ptout[gd.pt0].x), float(K.map_realposmin_z));  // max(zmax, DomPosMin.z)
        } else {
          r0 = gd.res[0];
          r1 = gd.res[1];
          r2 = gd.res[2];
        }
        gd.res[0] = r0;
        gd.res[1] = r1;
        gd.res[2] = r2;
        if (record) {
          gauge_set_timestep(s, t);
          if (gauge_output(s, t)) {
            emit = true;
            gauge_output_next(s, t);
          }
          gd.s = s;
        }
      }
    }
    // records in gauge order: the slot of each from the block-wide prefix of the emit flags
    const unsigned long long m = __ballot(emit);
    const unsigned pre = unsigned(__popcll(m & ((1ull << lane) - 1ull)));
    if (lane == 0) wtot[wave] = unsigned(__popcll(m));
    __syncthreads();
    unsigned off = nrec, tot = 0;
    for (unsigned k = 0; k < GW; k++) {
      if (k < wave) off += wtot[k];
      tot += wtot[k];
    }
    if (emit && off + pre < gs.reccap) {
      SphGaugeRecord rec;
      rec.time = t;
      rec.gauge = gi;
      rec.v[0] = r0;
      rec.v[1] = r1;
      rec.v[2] = r2;
      gs.rec[off + pre] = rec;
    }
    __syncthreads();
    if (tid == 0) nrec += tot;
    __syncthreads();
  }
  if (tid == 0 && record) {
    if (nrec > gs.reccap) {  // a full buffer drops the record; not fatal
      gs.ctl->dropped += nrec - gs.reccap;
      sc->error_flags |= ERR_GAUGE_FULL;
      nrec = gs.reccap;
    }
    gs.ctl->count = nrec;
  }
}

}  // namespace

void launch_gauge_eval(hipStream_t stm, const GaugeSet& gs, const DevScalars* sc, const PartArrays& a,
                       const unsigned* begincell, DivGrid g, const KConst& K, bool all) {
  if (gs.npts)
    hipLaunchKernelGGL(k_gauge_eval, dim3((gs.npts + GW - 1) / GW), dim3(GB), 0, stm, gs, sc, a, begincell, g, K, int(all));
  if (gs.nforce) hipLaunchKernelGGL(k_gauge_force, dim3(gs.nfblk), dim3(GB), 0, stm, gs, sc, a, begincell, g, K, int(all));
}

void launch_gauge_commit(hipStream_t stm, const GaugeSet& gs, DevScalars* sc, const KConst& K, bool record) {
  hipLaunchKernelGGL(k_gauge_commit, dim3(1), dim3(GB), 0, stm, gs, sc, K, int(record));
}

unsigned gauge_force_blocks(unsigned npbcap) { return npbcap ? (npbcap + GF_PART - 1) / GF_PART : 1u; }

}  // namespace sphx
