// internal.h -- error plumbing shared by the host sources of libmapsum (engine.cpp, ops.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mapsum.h"

inline thread_local std::string g_last_error;  // ms_last_error(nullptr)

struct MsError : std::runtime_error {
  int code;
  MsError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIP_OK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      throw MsError(MS_EIO, std::string(#expr) + ": " + hipGetErrorString(e_));             \
  } while (0)

#define REQUIRE(cond, code, msg)                      \
  do {                                                \
    if (!(cond)) throw MsError((code), (msg));        \
  } while (0)

// runs fn; an exception becomes its error code, with the text in e->err (if e) and g_last_error
template <class E, class Fn>
int guarded(E* e, Fn&& fn) {
  auto fail = [&](int code, const char* what) {
    if (e) e->err = what;
    g_last_error = what;
    return code;
  };
  try {
    return fn();
  } catch (const MsError& x) {
    return fail(x.code, x.what());
  } catch (const std::exception& x) {
    return fail(MS_EIO, x.what());
  } catch (...) {
    return fail(MS_EIO, "unknown exception");
  }
}
