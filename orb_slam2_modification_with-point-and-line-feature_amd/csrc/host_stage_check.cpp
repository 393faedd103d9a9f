// Stand-alone check of HostStage's sticky-failure path (make stage_check, host
// code under AddressSanitizer + UBSan). Meant for a machine without a device:
// there the first hipMalloc fails, which no GPU test can make happen. With a
// device present there is nothing to check and it says so.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_stage.h"

namespace {
int g_reports = 0, g_line = 0;
char g_what[64];
}  // namespace

// the library's reporter, replaced: counts the reports
int orbpl::hip_fail(hipError_t e, const char* what, int line) {
  g_reports++;
  g_line = line;
  snprintf(g_what, sizeof(g_what), "%s", what);
  printf("  reported: %s failed (line %d): %s\n", what, line, hipGetErrorString(e));
  return ORBPL_ERR_HIP;
}

#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      return 1;                                              \
    }                                                        \
  } while (0)

int main() {
  using orbpl::HostStage;
  {
    HostStage st;
    EXPECT(st.rc() == ORBPL_OK);
    const int first_line = __LINE__ + 1;
    float* a = st.out<float>(16);
    if (a) {
      printf("a device is present: hipMalloc succeeded, nothing to check\n");
      return 0;
    }
    // the first failure: reported once, with this file's line
    EXPECT(g_reports == 1 && g_line == first_line && !strcmp(g_what, "hipMalloc"));
    EXPECT(st.rc() == ORBPL_ERR_HIP);
    // every later allocation returns nullptr and reads no host memory: the
    // host pointers below are not readable
    const int* bad = reinterpret_cast<const int*>(uintptr_t(16));
    EXPECT(st.out<int>(0) == nullptr);
    EXPECT(st.zeros<int>(4) == nullptr);
    EXPECT(st.in(bad, 4, 8) == nullptr);
    EXPECT(st.in_opt(bad, 4, 8) == nullptr);
    EXPECT(st.in_opt(static_cast<const int*>(nullptr), 4, 8) == nullptr);
    EXPECT(st.in_value(7) == nullptr);
    const std::vector<double> v(5, 1.0);
    EXPECT(st.in(v) == nullptr);
    // back writes nothing and reads no device pointer; launched() stays quiet
    int host[4] = {-7, -7, -7, -7};
    st.back(host, bad, 4);
    std::vector<int> hv(3, -7);
    st.back(hv, bad);
    for (int x : host) EXPECT(x == -7);
    for (int x : hv) EXPECT(x == -7);
    EXPECT(st.launched() == ORBPL_ERR_HIP);
    EXPECT(st.rc() == ORBPL_ERR_HIP);
    EXPECT(g_reports == 1);
  }  // the destructor: nothing was allocated, nothing is freed
  EXPECT(g_reports == 1);
  {
    // a second stage starts clean and reports its own first failure, at the
    // line of the in() call that reached hipMalloc
    HostStage st;
    const int v = 3;
    const int line = __LINE__ + 1;
    EXPECT(st.in(&v, 1, 1) == nullptr);
    EXPECT(g_reports == 2 && g_line == line);
    const int* none = nullptr;
    EXPECT(st.in_opt(none, 0, 1) == nullptr && g_reports == 2);
  }
  printf("host_stage_check: ok\n");
  return 0;
}
