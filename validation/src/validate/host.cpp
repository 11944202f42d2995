// amdgpu-validate: what the Job asks of its host rather than of a GPU - the process
// start time, the node's preparation as the pod sees it, the Pushgateway POST.
#include "host.hpp"

#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include <netdb.h>
#include <sys/resource.h>
#include <sys/socket.h>
#include <unistd.h>

namespace ntm::job {

double process_start_epoch() {
  std::ifstream st("/proc/self/stat"), up("/proc/uptime");
  std::string s((std::istreambuf_iterator<char>(st)), std::istreambuf_iterator<char>());
  double uptime = 0;
  up >> uptime;
  const size_t rp = s.rfind(')');
  if (rp == std::string::npos || uptime <= 0) return wall_now();
  std::istringstream rest(s.substr(rp + 2));
  std::string tok;
  long long start_ticks = 0;
  for (int i = 0; i < 20 && rest >> tok; ++i)
    if (i == 19) start_ticks = std::atoll(tok.c_str());
  const long hz = sysconf(_SC_CLK_TCK);
  return wall_now() - uptime + (double)start_ticks / (double)hz;
}

HostPrep read_host_prep() {
  HostPrep h;
  std::ifstream nb("/proc/sys/kernel/numa_balancing");
  if (nb) nb >> h.numa_balancing;
  rlimit rl{};
  h.memlock_unlimited = getrlimit(RLIMIT_MEMLOCK, &rl) == 0 && rl.rlim_cur == RLIM_INFINITY;
  std::ifstream cl("/proc/cmdline");
  std::string w;
  while (cl >> w) h.iommu_pt = h.iommu_pt || w == "iommu=pt";
  return h;
}

// POST `body` (Prometheus text format) to a Pushgateway:
//   <url>/metrics/job/amdgpu_validate/instance/<host>
// Plain HTTP/1.1 over a socket (the image has no curl). Returns "ok" or a
// short error; never fatal - the verdict does not depend on the push.
std::string push_metrics(const std::string& url, const std::string& body) {
  const std::string scheme = "http://";
  if (url.rfind(scheme, 0) != 0) return "error: only http:// URLs";
  std::string rest = url.substr(scheme.size());
  const size_t slash = rest.find('/');
  std::string hostport = rest.substr(0, slash);
  std::string prefix = slash == std::string::npos ? "" : rest.substr(slash);
  while (!prefix.empty() && prefix.back() == '/') prefix.pop_back();
  std::string host = hostport, port = "9091";
  const size_t colon = hostport.rfind(':');
  if (colon != std::string::npos) {
    host = hostport.substr(0, colon);
    port = hostport.substr(colon + 1);
  }
  char me[256] = "unknown";
  gethostname(me, sizeof me - 1);
  const std::string path = prefix + "/metrics/job/amdgpu_validate/instance/" + me;
  addrinfo hints{}, *ai = nullptr;
  hints.ai_family = AF_UNSPEC;
  hints.ai_socktype = SOCK_STREAM;
  if (getaddrinfo(host.c_str(), port.c_str(), &hints, &ai) != 0 || !ai)
    return "error: cannot resolve " + host;
  int fd = -1;
  for (addrinfo* p = ai; p; p = p->ai_next) {
    fd = socket(p->ai_family, p->ai_socktype, p->ai_protocol);
    if (fd < 0) continue;
    timeval tv{10, 0};
    setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof tv);
    setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
    if (connect(fd, p->ai_addr, p->ai_addrlen) == 0) break;
    close(fd);
    fd = -1;
  }
  freeaddrinfo(ai);
  if (fd < 0) return "error: cannot connect to " + hostport;
  const std::string req = "POST " + path + " HTTP/1.1\r\nHost: " + hostport +
                          "\r\nContent-Type: text/plain; version=0.0.4\r\nContent-Length: " +
                          std::to_string(body.size()) + "\r\nConnection: close\r\n\r\n" + body;
  size_t off = 0;
  while (off < req.size()) {
    const ssize_t w = send(fd, req.data() + off, req.size() - off, MSG_NOSIGNAL);
    if (w <= 0) {
      close(fd);
      return "error: send failed";
    }
    off += (size_t)w;
  }
  char buf[256];
  const ssize_t r = recv(fd, buf, sizeof buf - 1, 0);
  close(fd);
  if (r <= 0) return "error: no response";
  buf[r] = 0;
  const std::string status(buf, strnlen(buf, sizeof buf));
  // "HTTP/1.1 200 OK" / "202 Accepted"
  if (status.size() > 12 && status[9] == '2') return "ok";
  return "error: " + status.substr(0, status.find('\r'));
}

}  // namespace ntm::job
