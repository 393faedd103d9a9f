// Stand-alone check of stereo_set_levels (make levels_check, host code under
// AddressSanitizer + UBSan): the level table of a StereoArgs on the stack is
// filled from real extractor geometries of 1, 8 and 16 levels; a write past
// the table is a sanitizer report. Needs no device.
#include <cstdio>
#include <cstring>

#include "orb_kernels.h"
#include "track_kernels.h"

#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      return 1;                                              \
    }                                                        \
  } while (0)

int main() {
  using namespace orbpl;
  const struct { int levels; float factor; } geoms[] = {{1, 1.2f}, {8, 1.2f}, {kMaxLevels, 1.05f}};
  for (const auto& c : geoms) {
    OrbHostGeom hg;
    const char* err = nullptr;
    EXPECT(build_orb_geometry(500, c.factor, c.levels, 321, 243, &hg, &err) == 0);
    // sentinels on both sides of the argument on the stack
    unsigned char before[64], after[64];
    memset(before, 0xA5, sizeof(before));
    StereoArgs a{};
    memset(after, 0x5A, sizeof(after));
    stereo_set_levels(a, hg.g);
    for (unsigned char b : before) EXPECT(b == 0xA5);
    for (unsigned char b : after) EXPECT(b == 0x5A);
    EXPECT(a.nrows == 243);
    for (int l = 0; l < kMaxLevels; l++) {
      const StereoLevel& s = a.lv[l];
      if (l >= c.levels) {
        EXPECT(s.w == 0 && s.h == 0 && s.off == 0);
        continue;
      }
      const LevelGeom& G = hg.g.lv[l];
      EXPECT(s.w == G.w && s.h == G.h && s.pitch == G.pitch && s.scale == G.scale);
      EXPECT(s.inv_scale == 1.0f / G.scale);
      EXPECT(s.off == content_off(G, 0, 0));
    }
    // the fields behind the table keep what the caller set
    EXPECT(a.entry_cap == 0 && a.err == nullptr && a.uright == nullptr);
  }
  // a kernel argument: well under the 4 KiB a launch accepts
  EXPECT(sizeof(StereoArgs) <= 1024);
  printf("stereo_levels_check: ok (StereoArgs %zu bytes)\n", sizeof(StereoArgs));
  return 0;
}
