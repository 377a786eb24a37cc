// gauge_sched_host.cpp — the gauge schedule of csrc/sph_gauge.hpp on the CPU.
//
// Reads from stdin: "ng nt", then per gauge "computestart computeend computedt outputsave
// outputstart outputend outputdt", then nt step times (any strtod form, e.g. hex floats).  Walks
// the times as the commit kernel does (Update -> SetTimeStep -> Output -> OutputNext) and prints,
// per gauge, one line with the indices of the times at which a record is stored.
#include <cstdio>
#include <cstdlib>
#include <vector>

#define SPH_GAUGE_SCHED_ONLY
#include "../../dualsphysics_multilayer_amd/csrc/sph_gauge.hpp"

int main() {
  unsigned ng = 0, nt = 0;
  if (std::scanf("%u %u", &ng, &nt) != 2) return 2;
  std::vector<sphx::GaugeSched> g(ng);
  char buf[7][64];
  for (unsigned i = 0; i < ng; i++) {
    if (std::scanf("%63s %63s %63s %63s %63s %63s %63s", buf[0], buf[1], buf[2], buf[3], buf[4], buf[5], buf[6]) != 7)
      return 2;
    sphx::GaugeSched s{};
    s.cstart = std::strtod(buf[0], nullptr);
    s.cend = std::strtod(buf[1], nullptr);
    s.cdt = std::strtod(buf[2], nullptr);
    s.osave = std::atoi(buf[3]);
    s.ostart = std::strtod(buf[4], nullptr);
    s.oend = std::strtod(buf[5], nullptr);
    s.odt = std::strtod(buf[6], nullptr);
    s.cnext = s.onext = 0;  // ConfigComputeTiming / ConfigOutputTiming
    g[i] = s;
  }
  std::vector<double> t(nt);
  for (unsigned k = 0; k < nt; k++) {
    if (std::scanf("%63s", buf[0]) != 1) return 2;
    t[k] = std::strtod(buf[0], nullptr);
  }
  for (unsigned i = 0; i < ng; i++) {
    sphx::GaugeSched& s = g[i];
    for (unsigned k = 0; k < nt; k++) {
      if (!sphx::gauge_update(s, t[k])) continue;
      sphx::gauge_set_timestep(s, t[k]);
      if (sphx::gauge_output(s, t[k])) {
        std::printf("%u ", k);
        sphx::gauge_output_next(s, t[k]);
      }
    }
    std::printf("\n");
  }
  return 0;
}
