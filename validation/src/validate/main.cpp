// amdgpu-validate: the post-provision validation Job entrypoint.
//
// Runs on the MI355X GPUs granted to the Kubernetes Job (amd.com/gpu: N) and
// proves them usable, replacing the NVIDIA GPU Operator's CUDA validator:
//
//   K1  hand-written bf16 MFMA GEMM per GPU (TFLOP/s + full verification
//       against an independent fp32 reference kernel)                    gpu.cpp
//   K2  HBM stream copy bandwidth + capacity check (288 GB class)        gpu.cpp
//   K4  HBM pattern test over (up to) all free HBM, off by default
//       (--hbm-test-gb; ntm/hbm_pattern.hpp)                             hbm_test.cpp
//   K5  per-CU compute sweep that names a bad CU, off by default
//       (--cu-sweep; ntm/cu_sweep.hpp)                                   cu_sweep.cpp
//   K6  host-link (PCIe) check: verified transfers both ways through pinned
//       host memory, rate and read latency, off by default
//       (--host-link-mib; ntm/host_link.hpp)                             host_link.cpp
//   K7  MX block-scaled matrix check: MXFP8 / MXFP6 / MXFP4 GEMMs with real
//       E8M0 scales, every element compared bitwise, off by default
//       (--mx-check; ntm/mx_gemm.hpp)                                    mx_check.cpp
//   K8  per-XCD sweep that names a slow or wrong XCD, off by default
//       (--xcd-sweep; ntm/xcd_sweep.hpp)                                 xcd_sweep.cpp
//   K9  atomics and cross-XCD hand-off check: every kind of global atomic with a
//       checked answer, plain stores handed between XCDs, off by default
//       (env NTM_ATOMICS_CHECK=1; ntm/atomics.hpp)                       atomics.cpp
//   K10 fp64 / fp32 / fp16 / int8 / 2:4-sparse matrix-core check: every matrix
//       instruction K1 and K7 never issue, exact answers, off by default
//       (env NTM_MCORE_CHECK=1; ntm/mcore.hpp)                           mcore.cpp
//   K11 MX quantise / dequantise on the device with the scaled-conversion
//       instructions, against integer reference kernels, off by default
//       (env NTM_MXQ_CHECK=1; ntm/mxq.hpp)                               mxq.cpp
//   K12 wave data paths (DPP, permutes, swizzle, lane swaps, transposed LDS
//       reads), the special-function unit and the gfx950 VALU additions, per
//       CU, off by default (env NTM_WAVE_CHECK=1; ntm/wave_paths.hpp)    wave.cpp
//   K13 fused attention forward (MFMA, row reduction, v_exp_f32, bf16 pack, second
//       MFMA in one loop): exact inputs bitwise against a reference kernel, dense
//       inputs within a derived tolerance, a rate, off by default
//       (env NTM_ATTN_CHECK=1; ntm/attn.hpp)                             attn.cpp
//   K14 paged-KV decode attention (block-table gather, split-KV, merge of partial
//       softmax state): exact inputs bitwise against K13's reference kernel on the
//       gathered keys, dense inputs within the derived tolerance, a KV read rate,
//       off by default (env NTM_PDA_CHECK=1; ntm/pda.hpp)                pda.cpp
//   C1  RCCL all-reduce sweep over xGMI (ncclCommInitAll, one process owns
//       all GPUs; every element checked)                                 collectives.hip
//   C2  hand-written two-shot all-reduce over peer-mapped xGMI, vs RCCL  collectives.hip
//   C3  per-link xGMI pull matrix                                        collectives.hip
//
// One process, one host thread per GPU for K1/K2 and the opt-in checks; no Python,
// no PyTorch - the container is small and starts fast (time-to-GPU-ready). Prints
// ONE JSON document; exit 0 = all checks passed, 1 = a check failed, 2 =
// environment error (no GPUs, not gfx950, HIP/RCCL error). README.md in this
// directory lists the places a new check touches.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <thread>

#include "check.hpp"
#include "host.hpp"
#include "sweeps.hpp"

using namespace ntm::job;

int main(int argc, char** argv) {
  Report R;
  R.t_start = process_start_epoch();
  Opts& o = R.o;
  if (!parse(argc, argv, o)) {
    usage();
    return 2;
  }
  if (!xgmi_knobs_ok(o)) return 2;
  if (o.describe_sweep) {  // host-only: the sweep definitions the GPU paths use, for CPU tests
    std::printf("%s\n", describe_sweep_json(o.allreduce_max_mib).c_str());
    return 0;
  }
  if (o.fault.empty())
    if (const char* f = std::getenv("NTM_FAULT_INJECT")) o.fault = f;
  if ((o.fault == "slow_xcd" || o.fault == "corrupt_xcd") && !o.xcd_sweep) {
    std::fprintf(stderr, "fault-inject %s needs --xcd-sweep\n", o.fault.c_str());
    usage();
    return 2;
  }
  if (const char* a = std::getenv("NTM_ATOMICS_CHECK")) o.atomics_check = std::string(a) == "1";
  if ((o.fault == "corrupt_atomic" || o.fault == "stale_handoff") && !o.atomics_check) {
    std::fprintf(stderr, "fault-inject %s needs NTM_ATOMICS_CHECK=1\n", o.fault.c_str());
    usage();
    return 2;
  }
  if (const char* a = std::getenv("NTM_MCORE_CHECK")) o.mcore_check = std::string(a) == "1";
  if (o.fault == "corrupt_mcore" && !o.mcore_check) {
    std::fprintf(stderr, "fault-inject corrupt_mcore needs NTM_MCORE_CHECK=1\n");
    usage();
    return 2;
  }
  if (const char* a = std::getenv("NTM_MXQ_CHECK")) o.mxq_check = std::string(a) == "1";
  if (o.fault == "corrupt_mxq" && !o.mxq_check) {
    std::fprintf(stderr, "fault-inject corrupt_mxq needs NTM_MXQ_CHECK=1\n");
    usage();
    return 2;
  }
  if (const char* a = std::getenv("NTM_WAVE_CHECK")) o.wave_check = std::string(a) == "1";
  if ((o.fault == "corrupt_wave" || o.fault == "corrupt_wave_sfu") && !o.wave_check) {
    std::fprintf(stderr, "fault-inject %s needs NTM_WAVE_CHECK=1\n", o.fault.c_str());
    usage();
    return 2;
  }
  if (const char* a = std::getenv("NTM_ATTN_CHECK")) o.attn_check = std::string(a) == "1";
  if (o.fault == "corrupt_attn" && !o.attn_check) {
    std::fprintf(stderr, "fault-inject corrupt_attn needs NTM_ATTN_CHECK=1\n");
    usage();
    return 2;
  }
  if (const char* a = std::getenv("NTM_PDA_CHECK")) o.pda_check = std::string(a) == "1";
  if (o.fault == "corrupt_pda" && !o.pda_check) {
    std::fprintf(stderr, "fault-inject corrupt_pda needs NTM_PDA_CHECK=1\n");
    usage();
    return 2;
  }
  // the Kubernetes node this ran on (NODE_NAME from the downward API in the
  // module's Job, one pod per GPU node): every verdict and metric names it
  if (const char* nn = std::getenv("NODE_NAME")) R.node = nn;

  R.hp = read_host_prep();
  if (o.require_host_prep || o.require_iommu_pt) {
    if (R.hp.numa_balancing != 0)
      fail("host prep: kernel.numa_balancing = " + std::to_string(R.hp.numa_balancing) + " (want 0)");
    if (!R.hp.memlock_unlimited) fail("host prep: RLIMIT_MEMLOCK is not unlimited (containerd LimitMEMLOCK)");
  }
  if (o.require_iommu_pt && !R.hp.iommu_pt) fail("host prep: iommu=pt missing from /proc/cmdline");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    const char* nn = std::getenv("NODE_NAME");
    std::printf("{\"passed\":false,%s\"failures\":[\"no AMD GPU visible\"]}\n",
                nn ? ("\"node\":" + jstr(nn) + ",").c_str() : "");
    return 2;
  }
  const int n = o.gpus > 0 ? std::min(o.gpus, ndev) : ndev;
  if (o.gpus > ndev) fail("requested " + std::to_string(o.gpus) + " GPUs, " + std::to_string(ndev) + " visible");
  R.devs.resize(n);
  for (int i = 0; i < n; ++i) R.devs[i] = i;
  R.t_hip = wall_now();

  // one thread per GPU: K1, K2 and the opt-in checks
  R.gpus.resize(n);
  std::vector<std::thread> th;
  for (int i = 0; i < n; ++i)
    th.emplace_back([&, i] { run_gpu(R.devs[i], i == n - 1, o, R.gpus[i]); });
  for (auto& t : th) t.join();
  for (auto& r : R.gpus)
    for (auto& f : gpu_failures(r, o)) fail(f);

  // C1 by default on n > 1; --rccl runs the one-rank communicator on n = 1 (the
  // same code path; its ~2 s RCCL init is not worth paying in a 1-GPU Job)
  if (o.rccl == 1 || (o.rccl < 0 && n > 1)) run_rccl(R.devs, o, R.rccl_rows);
  R.t_rccl = wall_now();
  if (o.xgmi && (n > 1 || o.xgmi_sim > 0)) run_xgmi(R.devs, o, R.xgmi_rows, R.xtune);
  if (o.p2p && (n > 1 || o.p2p_loopback)) run_p2p(R.devs, o, R.p2p);
  R.t_end = wall_now();
  // interconnect gates (0 = off; set from the first 8-GPU measurement)
  const double rccl_peak = peak_busbw(R.rccl_rows), xgmi_peak = peak_busbw(R.xgmi_rows);
  if (o.rccl_busbw_floor_gbps > 0 && !R.rccl_rows.empty() && rccl_peak < o.rccl_busbw_floor_gbps)
    fail("RCCL all-reduce peak bf16 busbw " + jnum(rccl_peak) + " GB/s below floor " +
         jnum(o.rccl_busbw_floor_gbps));
  if (o.xgmi_busbw_floor_gbps > 0 && !R.xgmi_rows.empty() && xgmi_peak < o.xgmi_busbw_floor_gbps)
    fail("xGMI all-reduce peak bf16 busbw " + jnum(xgmi_peak) + " GB/s below floor " +
         jnum(o.xgmi_busbw_floor_gbps));

  // the report: metrics (file, Pushgateway), the JSON document, the termination message
  R.failures = g_failures;
  const std::string prom_text = prometheus_text(R);
  if (!o.pushgateway.empty()) {
    R.push_status = push_metrics(o.pushgateway, prom_text);
    if (R.push_status != "ok") std::fprintf(stderr, "amdgpu-validate: pushgateway %s\n", R.push_status.c_str());
  }
  const std::string js = report_json(R);
  std::printf("%s\n", js.c_str());
  if (!o.out.empty()) std::ofstream(o.out) << js << "\n";
  if (!o.termination_log.empty()) std::ofstream(o.termination_log) << termination_message(R) << "\n";
  if (!o.prom_out.empty()) std::ofstream(o.prom_out) << prom_text;
  return R.passed() ? 0 : 1;
}
