// The host-side error state of a small library (scenes, augment, spatial): the thread's last message, the refusal macro of the
// entry points and the check after a launch.  Host code only.  Everything is in an anonymous namespace: each library is one
// translation unit and keeps a state of its own.  (The main library's as::err_buf / as::fail have external linkage across many
// translation units and stay in csrc/common.h and csrc/abi.hip.)
//
// This file is a shared header of the three libraries in anystereo/_srchash.py's table: an edit rebuilds and re-hashes all three,
// and — living below the top level of csrc/ — leaves the main library's hash alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

namespace {

char* err_buf() {
  static thread_local char buf[512] = "ok";
  return buf;
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

#define REQUIRE(cond, code, ...)                 \
  do {                                           \
    if (!(cond)) return fail(code, __VA_ARGS__); \
  } while (0)

// after a launch: 0, or `launch_code` (the library's *_ERR_LAUNCH) with the runtime's message
int check_launch(const char* what, int launch_code) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(launch_code, "%s: %s", what, hipGetErrorString(e));
  return 0;
}

}  // namespace
