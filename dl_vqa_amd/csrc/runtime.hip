// The library's runtime, compiled once: error buffer, dynamic-LDS attribute with the private-segment guard, VQA_* knobs, profiling
// hook, persistent-kernel slot count, the GEMM engines' split-K reduction kernels, and the C entry points about the library itself.
#include <stdarg.h>
#include <stdlib.h>

#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "gemm_host.hpp"

namespace vqa {

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return VQA_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return VQA_ERR_HIP;
}

// ------------------------------------------------------------------ launch plumbing
constexpr int kMaxScratchPerLane = 256;   // bytes; the shipped kernels use 0-200 (tests/test_abi_cpu.py checks the code objects)
static std::mutex g_attr_mu;
static std::set<std::pair<int, const void*>> g_attr_done;
int ensure_dyn_smem(const void* kernel, int bytes, const char* what) {
  int dev = 0;
  int rc = check_hip(hipGetDevice(&dev), "hipGetDevice");
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_attr_mu);
  if (g_attr_done.count({dev, kernel})) return VQA_OK;
  rc = check_hip(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), what);
  if (rc) return rc;
  // Private-segment guard (round-3 root cause of the round-2 hang): a workgroup-barrier kernel whose waves
  // need scratch deadlocked once ~2 000 of its waves (512 bytes per lane: ~64 MB of scratch) were dispatched -- 176
  // workgroups of 8 waves ran, 248 and more hung, whatever the problem shape; the same epilogue in a kernel with 100 bytes
  // per lane ran at any grid.  Every kernel of this library meets at workgroup barriers, so a kernel that comes out of the
  // compiler with a large private segment is refused here, before it can take a GPU down (VQA_ALLOW_SCRATCH=1: experiments).
  hipFuncAttributes attr;
  rc = check_hip(hipFuncGetAttributes(&attr, kernel), "hipFuncGetAttributes");
  if (rc) return rc;
  if (attr.localSizeBytes > kMaxScratchPerLane && !(getenv("VQA_ALLOW_SCRATCH") && atoi(getenv("VQA_ALLOW_SCRATCH")) == 1)) {
    set_error("%s: the kernel needs %zu bytes of scratch per lane (limit %d): refused -- workgroup-barrier kernels with a "
              "large private segment hang gfx950 beyond ~2000 resident waves (DESIGN.md 7(5))", what, (size_t)attr.localSizeBytes,
              kMaxScratchPerLane);
    return VQA_ERR_INVALID;
  }
  g_attr_done.insert({dev, kernel});
  return VQA_OK;
}

// Workgroups of `kernel` that are resident at once on the current device: min(planned, occupancy query) per CU x CUs.
// Cached per (device, kernel).  <= 0: the query failed (vqa_last_error says why).
int persistent_slots(const void* kernel, int threads, int smem_bytes, int planned_per_cu) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, int> cache;
  int dev = 0;
  if (check_hip(hipGetDevice(&dev), "hipGetDevice")) return -1;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_pair(dev, kernel);
  const auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0, cus = 0;
  if (check_hip(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, (size_t)smem_bytes),
                "hipOccupancyMaxActiveBlocksPerMultiprocessor(gemm_persistent)"))
    return -1;
  if (check_hip(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev), "hipDeviceGetAttribute(CUs)")) return -1;
  if (per_cu < 1) {
    set_error("gemm_persistent: the kernel does not fit a CU (occupancy query says %d workgroups)", per_cu);
    return -1;
  }
  const int slots = cus * (per_cu < planned_per_cu ? per_cu : planned_per_cu);
  cache[key] = slots;
  return slots;
}

// ------------------------------------------------------------------ knobs
static std::mutex g_knob_mu;
static Knobs g_knobs;
static bool g_knobs_read = false;
static int env_int(const char* name) {
  const char* e = getenv(name);
  return (e && *e) ? atoi(e) : -1;
}
static void read_knobs_locked() {
  g_knobs.split_target = env_int("VQA_SPLIT_TARGET");
  g_knobs.big_tiles = env_int("VQA_BIG_TILES");
  g_knobs.persistent = env_int("VQA_PERSISTENT");
  g_knobs.weight_stationary = env_int("VQA_WEIGHT_STATIONARY");
  g_knobs.wgrad_192 = env_int("VQA_WGRAD_192");
  g_knobs.wgrad_384 = env_int("VQA_WGRAD_384");
  g_knobs.conv_chunk = env_int("VQA_CONV_CHUNK");
  g_knobs.tall_bm = env_int("VQA_TALL_BM");
  g_knobs_read = true;
}
const Knobs& knobs() {
  std::lock_guard<std::mutex> lk(g_knob_mu);
  if (!g_knobs_read) read_knobs_locked();
  return g_knobs;
}

// ------------------------------------------------------------------ profiling hook
static std::mutex g_prof_mu;
static uint32_t g_prof_mask = 0;
static int g_prof_tag = -1;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_ev;
static std::vector<std::pair<int, int>> g_prof_key;   // (family, tag) of each recorded event pair
static thread_local int g_launch_tag = -1;
void set_launch_tag(int tag) { g_launch_tag = tag; }

ProfScope::ProfScope(int id_, hipStream_t s_) : id(id_), s(s_), on(false) {
  if (g_prof_mask == 0) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!((g_prof_mask >> id) & 1u) || (g_prof_tag >= 0 && g_prof_tag != g_launch_tag)) return;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;       // never inside a stream capture
  if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return;
  hipEvent_t a, b;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
  hipEventRecord(a, s);
  g_prof_ev.emplace_back(a, b);
  g_prof_key.emplace_back(id, g_launch_tag);
  on = true;
}
ProfScope::~ProfScope() {
  if (!on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  hipEventRecord(g_prof_ev.back().second, s);
}

// ------------------------------------------------------------------ split-K reduction (gemm.hip, gemm_x3.hip, bf16.hip)
__global__ void splitk_reduce_kernel(EpiParams pe, int splits) {
  const int64_t total = (int64_t)pe.M * pe.N;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int s = 0; s < splits; ++s) v += pe.slab[(int64_t)s * total + e];
    const int row = (int)(e / pe.N), col = (int)(e - (int64_t)row * pe.N);
    if (pe.aux) pe.aux[(int64_t)row * pe.ldc + col] = v;
    const float o = epi_apply(pe, v, row, col);
    if (pe.Cb) pe.Cb[(int64_t)row * pe.ldc + col] = epi_bf16(o); else pe.C[(int64_t)row * pe.ldc + col] = o;
  }
}

// N % 4 == 0: 16-byte slab reads; a block covers 64 float4 outputs with 4 thread groups that each take every 4th
// split, so all the loads of a thread are in flight at once (the scalar kernel above is a chain of dependent
// 4-byte loads: 16 us for an 8-split 256 x 1024 output), and the groups combine through LDS in a fixed order.
__global__ __launch_bounds__(256) void splitk_reduce4_kernel(EpiParams pe, int splits) {
  __shared__ float4 part[4][64];
  const int64_t total4 = (int64_t)pe.M * pe.N / 4;
  const int n4 = pe.N / 4;
  const float4* slab = reinterpret_cast<const float4*>(pe.slab);
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  for (int64_t e0 = (int64_t)blockIdx.x * 64; e0 < total4; e0 += (int64_t)gridDim.x * 64) {
    const int64_t e = e0 + lane;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < total4) {
      int s = grp;
      for (; s + 4 < splits; s += 8) {          // two independent loads per trip
        const float4 a = slab[(int64_t)s * total4 + e], b = slab[(int64_t)(s + 4) * total4 + e];
        v.x = (v.x + a.x) + b.x; v.y = (v.y + a.y) + b.y; v.z = (v.z + a.z) + b.z; v.w = (v.w + a.w) + b.w;
      }
      if (s < splits) {
        const float4 a = slab[(int64_t)s * total4 + e];
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
      }
    }
    part[grp][lane] = v;
    __syncthreads();
    if (grp == 0 && e < total4) {
      const float4 p1 = part[1][lane], p2 = part[2][lane], p3 = part[3][lane];
      const float r[4] = {(v.x + p1.x) + (p2.x + p3.x), (v.y + p1.y) + (p2.y + p3.y),
                          (v.z + p1.z) + (p2.z + p3.z), (v.w + p1.w) + (p2.w + p3.w)};
      const int row = (int)(e / n4), col = 4 * (int)(e - (int64_t)row * n4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (pe.aux) pe.aux[(int64_t)row * pe.ldc + col + k] = r[k];
        const float o = epi_apply(pe, r[k], row, col + k);
        if (pe.Cb) pe.Cb[(int64_t)row * pe.ldc + col + k] = epi_bf16(o); else pe.C[(int64_t)row * pe.ldc + col + k] = o;
      }
    }
    __syncthreads();
  }
}

int launch_splitk_reduce(const EpiParams& pe, int splits, hipStream_t s) {
  const bool vec = pe.N % 4 == 0;
  const int64_t total = (int64_t)pe.M * pe.N / (vec ? 4 : 1);
  int blocks = (int)((total + (vec ? 63 : 255)) / (vec ? 64 : 256));
  if (blocks > 4096) blocks = 4096;
  if (vec) hipLaunchKernelGGL(splitk_reduce4_kernel, dim3(blocks), dim3(256), 0, s, pe, splits);
  else hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, s, pe, splits);
  return check_hip(hipGetLastError(), "splitk_reduce launch");
}

#ifdef VQA_DIAG
unsigned long long* g_bar_dbg = nullptr;
#endif

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_abi_version(void) { return VQA_ABI_VERSION; }

#ifdef VQA_DIAG
/* diagnostic build only (tools/diag_barriers.py): device buffer of 4 x uint64 that the persistent GEMM kernels add their
 * per-role barrier counts to ([0] loader-wave barriers, [1] loader waves, [2] MFMA-wave barriers, [3] MFMA waves) */
int vqa_diag_barrier_buffer(void* dev_ptr) { g_bar_dbg = static_cast<unsigned long long*>(dev_ptr); return 0; }
#endif
const char* vqa_last_error(void) { return g_err; }

int vqa_device_ok(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 0;
  return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

int vqa_reload_knobs(void) {
  std::lock_guard<std::mutex> lk(g_knob_mu);
  read_knobs_locked();
  return VQA_OK;
}

int vqa_prof_arm_mask(uint32_t mask, int tag) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& e : g_prof_ev) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
  g_prof_ev.clear();
  g_prof_key.clear();
  g_prof_mask = mask;
  g_prof_tag = tag;
  return VQA_OK;
}

int vqa_prof_arm(int kernel_id, int tag) {
  const uint32_t all = (1u << VQA_K_COUNT) - 1u;
  return vqa_prof_arm_mask(kernel_id < 0 ? 0u : (kernel_id >= VQA_K_COUNT ? all : (1u << kernel_id)), tag);
}

int vqa_prof_read_groups(int* ids, int* tags, int* launches, float* total_ms, int cap) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  int n = 0;
  for (size_t e = 0; e < g_prof_ev.size(); ++e) {
    if (hipEventSynchronize(g_prof_ev[e].second) != hipSuccess) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_prof_ev[e].first, g_prof_ev[e].second) != hipSuccess) continue;
    int g = 0;
    while (g < n && g < cap && !(ids[g] == g_prof_key[e].first && tags[g] == g_prof_key[e].second)) ++g;
    if (g >= cap) continue;
    if (g == n) { ids[g] = g_prof_key[e].first; tags[g] = g_prof_key[e].second; launches[g] = 0; total_ms[g] = 0.f; ++n; }
    launches[g] += 1;
    total_ms[g] += ms;
  }
  return n;
}

int vqa_prof_read(int* launches, float* total_ms) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  float tot = 0.f;
  int n = 0;
  for (auto& e : g_prof_ev) {
    if (hipEventSynchronize(e.second) != hipSuccess) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) { tot += ms; ++n; }
  }
  if (launches) *launches = n;
  if (total_ms) *total_ms = tot;
  return VQA_OK;
}

}  // extern "C"
