// HIP_CHECK, and the device staging of the synchronous host-pointer entry
// points: Rows is one pitched column of such a call on the host, HostStage owns
// the device arrays of the call.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstddef>
#include <vector>

#include "../../include/orbpl.h"
#include "orbpl_runtime.h"

#define HIP_CHECK(expr)                                                \
  do {                                                                 \
    hipError_t _e = (expr);                                            \
    if (_e != hipSuccess) return orbpl::hip_fail(_e, #expr, __LINE__); \
  } while (0)

namespace orbpl {

// One column of a batched call: `rows` rows of `row` elements of T, every
// element `pad` until something fills it; d is the device array once a
// HostStage staged the column. The row length is stated here and nowhere else:
// put and take address a row by its number and refuse to pass its end.
template <class T>
struct Rows {
  size_t rows = 0, row = 0;
  std::vector<T> h;
  T* d = nullptr;

  Rows() = default;
  Rows(size_t rows_, size_t row_, T pad = T()) : rows(rows_), row(row_), h(rows_ * row_, pad) {}
  // element i of row r; at(p) is problem p's entry of a one-per-problem column
  T& at(size_t r, size_t i = 0) {
    assert(r < rows && i < row);
    return h[r * row + i];
  }
  // the first n elements of row r from src / to dst (NULL allowed when n == 0)
  void put(size_t r, const T* src, size_t n) {
    assert(n <= row && (n == 0 || r < rows));
    if (n) std::copy(src, src + n, h.begin() + r * row);
  }
  void take(size_t r, T* dst, size_t n) const {
    assert(n <= row && (n == 0 || r < rows));
    if (n) std::copy(h.begin() + r * row, h.begin() + r * row + n, dst);
  }
};

// One hipMalloc per array (an overrun faults instead of reaching a neighbour),
// blocking copies, counts and capacities in elements of T. The first HIP
// failure is reported once through hip_fail with the caller's line and is
// sticky: every later call does nothing, allocations return nullptr. An entry
// point checks rc() once before its launch and returns it at the end.
class HostStage {
 public:
  HostStage() = default;
  HostStage(const HostStage&) = delete;
  HostStage& operator=(const HostStage&) = delete;
  ~HostStage() {
    for (void* p : bufs_) (void)hipFree(p);
  }

  // an uninitialised array of cap elements
  template <class T>
  T* out(size_t cap, int line = __builtin_LINE()) {
    if (rc_) return nullptr;
    const size_t bytes = cap * sizeof(T);
    void* p = nullptr;
    if (!ok(hipMalloc(&p, bytes ? bytes : 1), "hipMalloc", line)) return nullptr;
    bufs_.push_back(p);
    return static_cast<T*>(p);
  }
  template <class T>
  T* zeros(size_t cap, int line = __builtin_LINE()) {
    T* d = out<T>(cap, line);
    if (d) ok(hipMemset(d, 0, cap * sizeof(T)), "hipMemset", line);
    return rc_ ? nullptr : d;
  }
  // cap elements, the first n copied from h (h may be NULL when n == 0)
  template <class T>
  T* in(const T* h, size_t n, size_t cap, int line = __builtin_LINE()) {
    T* d = out<T>(cap, line);
    if (d && n) ok(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy to device", line);
    return rc_ ? nullptr : d;
  }
  template <class T>
  T* in(const std::vector<T>& h, int line = __builtin_LINE()) {
    return in(h.data(), h.size(), h.size(), line);
  }
  template <class T>
  T* in_value(const T& v, int line = __builtin_LINE()) {
    return in(&v, 1, 1, line);
  }
  // an optional input: no array when the caller passed none
  template <class T>
  T* in_opt(const T* h, size_t n, size_t cap, int line = __builtin_LINE()) {
    return h ? in(h, n, cap, line) : nullptr;
  }
  template <class T>
  void back(T* h, const T* d, size_t n, int line = __builtin_LINE()) {
    if (rc_ || !n) return;
    ok(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy to host", line);
  }
  template <class T>
  void back(std::vector<T>& h, const T* d, int line = __builtin_LINE()) {
    back(h.data(), d, h.size(), line);
  }
  // a column: staged from (in), sized as (out), zeroed as (zeros) or copied back
  // into (back) its host vector. out, zeros and inout remember the column:
  // back_outs copies every remembered column back
  template <class T>
  T* in(Rows<T>& c, int line = __builtin_LINE()) {
    return c.d = in(c.h, line);
  }
  template <class T>
  T* inout(Rows<T>& c, int line = __builtin_LINE()) {
    outs_.push_back({c.h.data(), in(c, line), c.h.size() * sizeof(T)});
    return c.d;
  }
  template <class T>
  T* out(Rows<T>& c, int line = __builtin_LINE()) {
    outs_.push_back({c.h.data(), c.d = out<T>(c.h.size(), line), c.h.size() * sizeof(T)});
    return c.d;
  }
  template <class T>
  T* zeros(Rows<T>& c, int line = __builtin_LINE()) {
    outs_.push_back({c.h.data(), c.d = zeros<T>(c.h.size(), line), c.h.size() * sizeof(T)});
    return c.d;
  }
  template <class T>
  void back(Rows<T>& c, int line = __builtin_LINE()) {
    back(c.h, c.d, line);
  }
  void back_outs(int line = __builtin_LINE()) {
    for (const Out& o : outs_) back(static_cast<char*>(o.h), static_cast<const char*>(o.d), o.bytes, line);
  }
  // after the launch: folds in hipGetLastError()
  int launched(int line = __builtin_LINE()) {
    if (!rc_) ok(hipGetLastError(), "hipGetLastError()", line);
    return rc_;
  }
  int rc() const { return rc_; }

 private:
  bool ok(hipError_t e, const char* what, int line) {
    if (e != hipSuccess) rc_ = hip_fail(e, what, line);
    return e == hipSuccess;
  }
  struct Out {
    void* h;
    const void* d;
    size_t bytes;
  };
  std::vector<void*> bufs_;
  std::vector<Out> outs_;
  int rc_ = ORBPL_OK;
};

}  // namespace orbpl
