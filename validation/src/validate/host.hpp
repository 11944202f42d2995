// amdgpu-validate: host-side helpers of main (host.cpp).
#pragma once

#include <chrono>
#include <string>

#include "report.hpp"

namespace ntm::job {

// epoch seconds, now
inline double wall_now() {
  return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
}

// epoch seconds at which this process started (/proc/self/stat), now if unreadable
double process_start_epoch();

HostPrep read_host_prep();

// POST `body` (Prometheus text format) to a Pushgateway; "ok" or a short error, never fatal
std::string push_metrics(const std::string& url, const std::string& body);

}  // namespace ntm::job
