// devmem_host.cpp — the capacity rule of csrc/sph_devmem.hpp on the CPU.
//
// grown_capacity against a literal table (the rule of every growing buffer: the slab send and
// receive buffers, the face records, the RCCL gather scratch), so that a change of the rule is
// noticed.  Exit status 0 when every row holds; the rows that do not are printed.
#include <cstdio>

#define SPH_DEVMEM_CAPACITY_ONLY
#include "../../dualsphysics_multilayer_amd/csrc/sph_devmem.hpp"

int main() {
  struct Row {
    unsigned long long need, floor;
    bool exact;
    unsigned long long want;
  };
  const Row rows[] = {
      {0, 4096, false, 4096},
      {1, 1024, false, 1025},
      {3, 1024, false, 1028},
      {100000, 4096, false, 154096},
      {7, 4096, true, 7},
      {(1ull << 40) + 1, 1024, false, (1ull << 40) + (1ull << 39) + 1025},
  };
  static_assert(sphx::grown_capacity(3, 1024, false) == 1028, "usable in constant expressions");
  int bad = 0;
  for (const Row& r : rows) {
    const unsigned long long got = sphx::grown_capacity(r.need, r.floor, r.exact);
    if (got == r.want) continue;
    std::printf("grown_capacity(%llu, %llu, %d) = %llu, expected %llu\n", r.need, r.floor, int(r.exact), got, r.want);
    bad++;
  }
  std::printf("%d of %zu rows differ\n", bad, sizeof(rows) / sizeof(rows[0]));
  return bad ? 1 : 0;
}
