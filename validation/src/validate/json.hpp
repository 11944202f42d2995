// amdgpu-validate: the two JSON value writers every output goes through (host-only).
#pragma once

#include <cmath>
#include <cstdio>
#include <string>

namespace ntm::job {

// a number, or null where JSON has no word for it (NaN, infinity)
inline std::string jnum(double v) {
  if (!std::isfinite(v)) return "null";
  char b[64];
  std::snprintf(b, sizeof b, "%.15g", v);
  return b;
}

// a string: quote and backslash escaped, control characters dropped
inline std::string jstr(const std::string& s) {
  std::string o = "\"";
  for (char c : s) {
    if (c == '"' || c == '\\') o += '\\';
    if ((unsigned char)c < 0x20) continue;
    o += c;
  }
  return o + "\"";
}

inline const char* jbool(bool b) { return b ? "true" : "false"; }

}  // namespace ntm::job
