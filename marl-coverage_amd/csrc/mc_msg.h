// mc_msg.h — printf into a std::string: the one formatter of the host's error
// messages (mc_host.h fail; the pure checks of mc_config.h and mc_beams.h,
// which hand their message back).  Host-only, no HIP call.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <string>

namespace mc {
// (formats into a buffer of its own first: an argument may point into `err`)
inline void vmsgf(std::string& err, const char* fmt, va_list ap) {
  char buf[512];
  vsnprintf(buf, sizeof(buf), fmt, ap);
  err = buf;
}
// sets `err` and returns false, so a check reads `return msgf(err, ...)`
__attribute__((format(printf, 2, 3))) inline bool msgf(std::string& err, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vmsgf(err, fmt, ap);
  va_end(ap);
  return false;
}
}  // namespace mc
