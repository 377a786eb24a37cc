// sph_solver_impl.hpp — what the sph_solver*.cpp files share besides the class itself: the
// derived constants of sph_constants.cpp and the slab protocol's trace.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sph_solver.hpp"

namespace sphx {

// sph_constants.cpp (pure host arithmetic)
unsigned bits_for(unsigned v, unsigned minbits);
KConst make_kconst(const SphConstants& c);
PeriConst make_periconst(const SphConstants& c);
DivGrid make_grid(const SphConstants& c, const SlabConfig* slab);
unsigned initial_periodic_count(const SphConstants& C, const SphParticlesHost& h, unsigned npb);
std::vector<unsigned> initial_columns(const SphConstants& C, const SphParticlesHost& h, int axis);

// SPH_TRACE_SLAB=1: one stderr line per slab phase (rank, step, phase) -- a diagnostic of the
// slab protocol's host side (which rank waits where)
inline bool trace_slab() {
  static const bool on = [] {
    const char* e = std::getenv("SPH_TRACE_SLAB");
    return e && *e == '1';
  }();
  return on;
}
#define SLAB_TRACE(what)                                                                                     \
  do {                                                                                                      \
    if (trace_slab() && slab())                                                                             \
      std::fprintf(stderr, "slabtrace rank %d step %llu %s\n", slabcfg_.rank, stepsdone_, what);          \
  } while (0)

}  // namespace sphx
