// amdgpu-validate: the C1 / C2 message-size lists and the busbw factor (host-only).
// --describe-sweep prints them without touching a GPU, so a CPU test can hold the
// torch sweeps of parallel/collectives.py to them.
#pragma once

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include "json.hpp"

namespace ntm::job {

inline double bus_factor(int n) { return n > 1 ? 2.0 * (n - 1) / n : 0.0; }

// C1 message sizes up to maxb: nccl-tests style, 8 B .. max, x4 per step (the
// torch sweep in parallel/collectives.py builds the same list; a CPU test
// pins the two against each other through --describe-sweep)
inline std::vector<size_t> rccl_sizes(size_t maxb) {
  std::vector<size_t> v;
  for (size_t b = 8; b <= maxb; b *= 4) v.push_back(b);
  return v;
}

// C2 message sizes: the C1 sizes from 512 B that split into 8-element chunks
// per rank, so every C2 row pairs with a C1 row (bench.py builds the same list)
inline std::vector<size_t> xgmi_sizes(size_t maxb, int n) {
  std::vector<size_t> v;
  for (const size_t b : rccl_sizes(maxb))
    if (b >= 512 && (b / 2) % (8 * (size_t)n) == 0) v.push_back(b);
  return v;
}

// --describe-sweep: the sweep definitions the GPU paths use, as one JSON line
inline std::string describe_sweep_json(long allreduce_max_mib) {
  const size_t maxb = (size_t)allreduce_max_mib << 20;
  auto arr = [](const std::vector<size_t>& v) {
    std::string t = "[";
    for (size_t i = 0; i < v.size(); ++i) t += (i ? "," : "") + std::to_string(v[i]);
    return t + "]";
  };
  std::string t = "{\"rccl_bytes\":" + arr(rccl_sizes(maxb)) + ",\"bus_factor\":[";
  for (int k = 1; k <= 8; ++k) t += (k > 1 ? "," : "") + jnum(bus_factor(k));
  t += "],\"xgmi_bytes\":{";
  for (int k = 1; k <= 8; ++k)
    t += (k > 1 ? ",\"" : "\"") + std::to_string(k) + "\":" + arr(xgmi_sizes(std::min<size_t>(maxb, (size_t)1 << 30), k));
  return t + "}}";
}

}  // namespace ntm::job
