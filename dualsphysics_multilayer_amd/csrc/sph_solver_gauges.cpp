// sph_solver_gauges.cpp — SphGpuSingle: the gauges (sph_gauge.hip).
#include "sph_solver.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace sphx {

// ---- gauges (sph_gauge.hip) ----------------------------------------------------------------
// The due gauges on the updated particles with the cell table of the last divide (begincell_
// and the sorted order stay as that divide left them until RunCellDivide: the update kernels,
// with or without the fused classification, write particle data and the next divide's scratch
// only), then the results, schedules and records.
void SphGpuSingle::RunGauges() {
  launch_gauge_eval(stream, gauges_, sc_, cur_, begincell_, G, K, false);
  launch_gauge_commit(stream, gauges_, sc_, K, true);
}

void SphGpuSingle::SetGauges(unsigned n, const SphGaugeDef* defs, unsigned record_capacity) {
  if (slab()) throw SphError(SPH_ERR_UNSUPPORTED, "gauges run on a single domain only (not on slabs)");
  if (peri_) throw SphError(SPH_ERR_UNSUPPORTED, "gauges with periodic boundaries are not implemented");
  if (inout_) throw SphError(SPH_ERR_UNSUPPORTED, "gauges with inlet/outlet zones are not implemented");
  if (nn_) throw SphError(SPH_ERR_UNSUPPORTED, "gauges with NN multiphase are not implemented");
  if (stepped_ || gauges_.ng) throw SphError(SPH_ERR_STATE, "the gauges are configured once, before the first step");
  if (!n || !defs) throw SphError(SPH_ERR_ARG, "no gauges");
  if (!record_capacity) throw SphError(SPH_ERR_ARG, "the gauge record buffer needs a capacity");
  std::vector<GaugeDev> gd(n);
  std::vector<GaugePoint> pts;
  std::vector<unsigned> fidx;
  for (unsigned i = 0; i < n; i++) {
    const SphGaugeDef& d = defs[i];
    GaugeDev& g = gd[i];
    std::memset(&g, 0, sizeof(g));
    // ConfigComputeTiming / ConfigOutputTiming (JDsGaugeItem.cpp:113-129): both Next start at 0
    g.s.cstart = d.computestart;
    g.s.cend = d.computeend;
    g.s.cdt = d.computedt;
    g.s.ostart = d.outputstart;
    g.s.oend = d.outputend;
    g.s.odt = d.outputdt;
    g.s.osave = d.output ? 1 : 0;
    if (!(d.computedt >= 0) || !(d.outputdt >= 0)) throw SphError(SPH_ERR_ARG, "gauge: negative computedt / outputdt");
    g.type = d.type;
    g.pt0 = unsigned(pts.size());
    for (int k = 0; k < 3; k++) {
      g.p0[k] = d.point0[k];
      g.dir[k] = d.pointdir[k];
    }
    switch (d.type) {
      case SPH_GAUGE_VEL:
        g.npt = 1;
        pts.push_back(GaugePoint{d.point0[0], d.point0[1], d.point0[2], i, 0u});
        break;
      case SPH_GAUGE_SWL: {
        if (!(d.masslimit > 0)) throw SphError(SPH_ERR_ARG, "gauge: the masslimit is invalid");
        if (d.pointnp > (1u << 20)) throw SphError(SPH_ERR_ARG, "gauge: too many SWL points");
        g.pointnp = d.pointnp;
        g.masslimit = d.masslimit;
        g.npt = d.pointnp + 1;
        // the points as JGaugeSwl::CalculeCpuT walks them: ptpos = ptpos + PointDir
        double p[3] = {d.point0[0], d.point0[1], d.point0[2]};
        for (unsigned k = 0; k <= d.pointnp; k++) {
          pts.push_back(GaugePoint{p[0], p[1], p[2], i, k});
          for (int c = 0; c < 3; c++) p[c] = p[c] + d.pointdir[c];
        }
        break;
      }
      case SPH_GAUGE_MAXZ:
        if (!(d.distlimit > 0)) throw SphError(SPH_ERR_ARG, "gauge: the distlimit is invalid");
        g.height = d.height;
        g.distlimit = d.distlimit;
        g.npt = 1;
        pts.push_back(GaugePoint{d.point0[0], d.point0[1], d.point0[2], i, 0u});
        break;
      case SPH_GAUGE_FORCE: {
        // JGaugeSystem::AddGaugeForce (JDsGaugeSystem.cpp:345): fixed or moving blocks only
        const unsigned type = d.code & unsigned(CODE_MASKTYPE);
        if ((d.code & ~unsigned(CODE_MASKTYPE | CODE_MASKVALUE)) || (type != 0u && type != unsigned(CODE_TYPE_MOVING)))
          throw SphError(SPH_ERR_UNSUPPORTED,
                         "Type of boundary particles is invalid. Only fixed or moving particles are allowed.");
        g.code = d.code;
        g.fslot = unsigned(fidx.size());
        fidx.push_back(i);
        break;
      }
      default:
        throw SphError(SPH_ERR_ARG, "gauge type is invalid");
    }
  }
  check_hip(hipSetDevice(device), "hipSetDevice");
  GaugeSet gs;
  gs.npts = unsigned(pts.size());
  gs.nforce = unsigned(fidx.size());
  gs.nfblk = gauge_force_blocks(npb0_);
  gs.reccap = record_capacity;
  gs.gauges = allocs_.upload(gd.data(), n);
  gs.pts = allocs_.upload(pts.data(), pts.size());
  gs.ptout = allocs_.alloc<double4>(std::max<size_t>(pts.size(), 1));
  gs.fidx = allocs_.upload(fidx.data(), fidx.size());
  gs.fpart = allocs_.alloc<double>(3 * size_t(gs.nfblk) * std::max<size_t>(fidx.size(), 1));
  gs.rec = allocs_.alloc<SphGaugeRecord>(record_capacity);
  gs.ctl = allocs_.alloc<GaugeCtl>(1);
  check_hip(hipMemset(gs.ptout, 0, sizeof(double4) * std::max<size_t>(pts.size(), 1)), "zero gauge sums");
  check_hip(hipMemset(gs.fpart, 0, 8 * 3 * size_t(gs.nfblk) * std::max<size_t>(fidx.size(), 1)), "zero gauge sums");
  check_hip(hipMemset(gs.ctl, 0, sizeof(GaugeCtl)), "zero gauge records");
  gs.ng = n;
  gauges_ = gs;
  // RunGaugeSystem(TimeStep, true) before the loop (JSphCpuSingle.cpp:1070): the freshly
  // divided state at the current TimeStep
  RunGauges();
  Sync();
  check_hip(hipGetLastError(), "gauge kernels");
}

unsigned SphGpuSingle::GaugeRecords(SphGaugeRecord* out, unsigned cap) {
  if (!gauges_.ng) throw SphError(SPH_ERR_STATE, "no gauges are configured");
  Sync();
  GaugeCtl ctl;
  check_hip(hipMemcpy(&ctl, gauges_.ctl, sizeof(ctl), hipMemcpyDeviceToHost), "read gauge records");
  if (!out) return ctl.count;
  if (cap < ctl.count) throw SphError(SPH_ERR_ARG, "gauge record buffer too small");
  if (ctl.count)
    check_hip(hipMemcpy(out, gauges_.rec, sizeof(SphGaugeRecord) * size_t(ctl.count), hipMemcpyDeviceToHost),
              "read gauge records");
  check_hip(hipMemset(gauges_.ctl, 0, sizeof(GaugeCtl)), "zero gauge records");
  return ctl.count;
}

void SphGpuSingle::Measure(SphGaugeRecord* out, unsigned n) {
  if (!gauges_.ng) throw SphError(SPH_ERR_STATE, "no gauges are configured");
  if (n != gauges_.ng || !out) throw SphError(SPH_ERR_ARG, "one output record per gauge is needed");
  check_hip(hipSetDevice(device), "hipSetDevice");
  launch_gauge_eval(stream, gauges_, sc_, cur_, begincell_, G, K, true);
  launch_gauge_commit(stream, gauges_, sc_, K, false);
  const SphRunStats st = Stats();  // synchronises
  std::vector<GaugeDev> gd(n);
  check_hip(hipMemcpy(gd.data(), gauges_.gauges, sizeof(GaugeDev) * n, hipMemcpyDeviceToHost), "read gauges");
  for (unsigned i = 0; i < n; i++) {
    out[i].time = st.time;
    out[i].gauge = i;
    for (int k = 0; k < 3; k++) out[i].v[k] = gd[i].res[k];
  }
}

}  // namespace sphx
