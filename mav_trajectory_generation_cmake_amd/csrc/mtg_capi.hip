// mtg_capi.hip -- the C ABI (include/mtg.h): contexts, staging, launches.
// Never aborts, never throws across the boundary; errors are return codes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <pthread.h>
#include <sched.h>

#include <cctype>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "mtg.h"
#include "mtg_internal.h"
#include "mtg_ragged_plan.h"

// A persistent host thread of a context that runs one job at a time for the caller (the pipelined
// solve's D2H issuer): created on first use and kept, instead of a std::thread per call (~50-100 us of
// thread creation per host-array solve), and bound to the CPUs of the GPU's NUMA node where the
// process may run there (the pageable-copy staging and completion waits then stay node-local).
struct CtxWorker {
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  std::function<void()> job;
  bool has_job = false, quit = false;
  ~CtxWorker() {
    if (!th.joinable()) return;
    {
      std::lock_guard<std::mutex> g(m);
      quit = true;
    }
    cv.notify_all();
    th.join();
  }
  // start the thread (once); false if no thread can be created
  bool start(const cpu_set_t* affinity) {
    if (th.joinable()) return true;
    try {
      th = std::thread([this] {
        std::unique_lock<std::mutex> l(m);
        for (;;) {
          cv.wait(l, [this] { return has_job || quit; });
          if (quit) return;
          std::function<void()> j = std::move(job);
          l.unlock();
          j();
          l.lock();
          has_job = false;
          cv.notify_all();
        }
      });
    } catch (...) {
      return false;
    }
    if (affinity) (void)pthread_setaffinity_np(th.native_handle(), sizeof(cpu_set_t), affinity);
    return true;
  }
  void post(std::function<void()> j) {
    std::lock_guard<std::mutex> g(m);
    job = std::move(j);
    has_job = true;
    cv.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> l(m);
    cv.wait(l, [this] { return !has_job; });
  }
};

struct mtg_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  void* staging = nullptr;
  size_t staging_bytes = 0;
  void* workspace = nullptr;
  size_t workspace_bytes = 0;
  void* pinned = nullptr;  // host mirror of the staging layout for small calls (hipHostMalloc)
  size_t pinned_bytes = 0;
  // ring of (start, stop) events around kernel launches; launches counts recorded launches
  std::vector<hipEvent_t> ev_start, ev_stop;
  int64_t launches = 0;
  std::string last_error;
  std::mutex mu;
  int inject_rc = 0;  // mtg_debug_fail_next_solve: the next solve's return code (0: none)
  // Pipelined host-pointer solves (run_solve_pipelined): kPipeSlots chunks in flight, each with its
  // own kernel stream and device buffers; all H2D copies go through one stream and all D2H copies
  // through another (one copy queue per direction).
  static constexpr int kPipeSlots = 4;
  struct PipeSlot {
    hipStream_t stream = nullptr;  // the chunk's kernel
    hipEvent_t in_done = nullptr;  // its H2D copies landed (recorded on pipe_h2d)
    hipEvent_t k_done = nullptr;   // its kernel finished (recorded on stream)
    hipEvent_t done = nullptr;     // its D2H copies landed (recorded on pipe_d2h)
    void* dev = nullptr;  // device inputs + outputs of one chunk
    size_t dev_bytes = 0;
  } pipe[kPipeSlots];
  hipStream_t pipe_h2d = nullptr, pipe_d2h = nullptr;
  hipEvent_t pipe_start = nullptr;
  CtxWorker d2h_worker;
  // Ragged solves (run_solve_ragged): the device copy of the plan records and the packed arrays of the
  // gathered groups.  Not ctx->workspace: the DLX and split kernels use that during the same call.
  void* ragged = nullptr;
  size_t ragged_bytes = 0;
  // the records are uploaded from pinned memory the context owns (an asynchronous copy outlives the
  // call); two buffers taken in turn, each reused only after the event behind its last upload
  struct RaggedHost {
    void* p = nullptr;
    size_t bytes = 0;
    hipEvent_t uploaded = nullptr;
    bool pending = false;
  } ragged_host[2];
  int ragged_turn = 0;
  hipEvent_t ragged_done = nullptr;  // the last ragged call's last kernel (it may have run on another stream)
  bool ragged_done_pending = false;
};

namespace mtg {
PendingEvents& pending_events() {
  static thread_local PendingEvents pe;
  return pe;
}
}  // namespace mtg

namespace {

int set_hip_error(mtg_ctx* ctx, hipError_t e, const char* what) {
  if (ctx) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    ctx->last_error = buf;
  }
  return e == hipErrorOutOfMemory ? MTG_ERR_OUT_OF_MEMORY : MTG_ERR_HIP;
}

int set_error(mtg_ctx* ctx, int code, const char* what) {
  if (ctx) ctx->last_error = what;
  return code;
}

#define MTG_HIP_TRY(ctx, expr)                          \
  do {                                                  \
    hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) return set_hip_error(ctx, e_, #expr); \
  } while (0)

size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

size_t grid_bytes(const mtg_sdf_grid& g) { return sizeof(float) * (size_t)g.nx * g.ny * g.nz; }

// host-pointer calls whose staged arrays fit this size go through one pinned buffer
constexpr size_t kPinnedMax = 1u << 20;

hipError_t ensure(void** buf, size_t* have, size_t need) {
  if (*have >= need) return hipSuccess;
  if (*buf) {
    hipError_t e = hipFree(*buf);
    if (e != hipSuccess) return e;
    *buf = nullptr;
    *have = 0;
  }
  hipError_t e = hipMalloc(buf, need);
  if (e == hipSuccess) *have = need;
  return e;
}

// The arrays of one call.  Each array is registered once, with the pointer the launch will use:
// *dev is the caller's pointer at once, and stays so in a device-pointer call (MTG_FLAG_DEVICE_PTRS),
// also where 0 bytes are registered.  In a host-pointer call upload() gives every array with bytes and
// a host pointer a 256-B aligned slot of ctx->staging (inputs first, each group in registration
// order), sizes the buffer, and only then points *dev into it (nullptr for the others) and queues the
// H2D copy of each input; finish() queues the D2H copy of each output and waits for the stream.  A
// device-pointer call's finish() waits unless MTG_FLAG_ASYNC.  Everything goes on ctx->stream; the
// memsets, the timed region and the launches stay with the caller, between the two.  Both return an
// MTG_* code with mtg_last_error set.
class Staged {
 public:
  Staged(mtg_ctx* ctx, unsigned flags) : ctx_(ctx), dev_(flags & MTG_FLAG_DEVICE_PTRS), async_(flags & MTG_FLAG_ASYNC) {}
  template <class T>
  void in(const T** dev, const T* host, size_t bytes) {
    *dev = host;
    add(dev, const_cast<T*>(host), bytes, kIn);
  }
  template <class T>
  void out(T** dev, T* host, size_t bytes) {
    *dev = host;
    add(dev, host, bytes, kOut);
  }
  template <class T>
  void inout(T** dev, T* host, size_t bytes) {
    *dev = host;
    add(dev, host, bytes, kIn | kOut);
  }

  int upload() {
    if (overflow_) return set_error(ctx_, MTG_ERR_INVALID_ARGUMENT, "internal: a call stages more arrays than Staged holds");
    if (dev_) return MTG_OK;
    size_t off = 0;
    for (unsigned pass : {kIn, 0u})
      for (int i = 0; i < n_; ++i)
        if ((rec_[i].dir & kIn) == pass) {
          rec_[i].off = off;
          off = align_up(off + rec_[i].bytes);
        }
    hipError_t e = ensure(&ctx_->staging, &ctx_->staging_bytes, std::max<size_t>(off, 256));
    if (e != hipSuccess) return set_hip_error(ctx_, e, "stage inputs: ensure(staging)");
    for (int i = 0; i < n_; ++i) {
      const Rec& r = rec_[i];
      void* p = r.bytes ? static_cast<char*>(ctx_->staging) + r.off : nullptr;
      std::memcpy(r.dev, &p, sizeof(p));  // (every *dev is an object pointer)
      if (r.bytes && (r.dir & kIn)) {
        e = hipMemcpyAsync(p, r.host, r.bytes, hipMemcpyHostToDevice, ctx_->stream);
        if (e != hipSuccess) return set_hip_error(ctx_, e, "stage inputs");
      }
    }
    return MTG_OK;
  }

  int finish() {
    if (dev_ && async_) return MTG_OK;
    for (int i = 0; !dev_ && i < n_; ++i) {
      const Rec& r = rec_[i];
      if (!r.bytes || !(r.dir & kOut)) continue;
      hipError_t e = hipMemcpyAsync(r.host, static_cast<char*>(ctx_->staging) + r.off, r.bytes, hipMemcpyDeviceToHost,
                                    ctx_->stream);
      if (e != hipSuccess) return set_hip_error(ctx_, e, "copy outputs");
    }
    MTG_HIP_TRY(ctx_, hipStreamSynchronize(ctx_->stream));
    return MTG_OK;
  }

 private:
  static constexpr unsigned kIn = 1, kOut = 2;
  static constexpr int kMax = 16;  // (mtg_objective_time_batch stages 14)
  struct Rec {
    void* dev;   // the caller's T* variable
    void* host;
    size_t bytes, off;
    unsigned dir;
  };
  void add(void* dev, void* host, size_t bytes, unsigned dir) {
    if (n_ < kMax) rec_[n_++] = Rec{dev, host, host ? bytes : 0, 0, dir};
    else overflow_ = true;  // upload() reports it
  }
  mtg_ctx* ctx_;
  bool dev_, async_, overflow_ = false;
  int n_ = 0;
  Rec rec_[kMax];
};

// Timed region around one launch.  single: the call launches exactly one kernel through
// mtg::launch_kernel, which carries the event pair in its dispatch packet; otherwise (the split
// path's two kernels) the events are recorded as stream markers around the launches.
hipError_t time_begin(mtg_ctx* ctx, bool single = true) {
  mtg::PendingEvents& pe = mtg::pending_events();
  pe = mtg::PendingEvents{};
  if (ctx->ev_start.empty()) return hipSuccess;  // timing disabled (mtg_enable_timing(ctx, 0))
  const size_t slot = (size_t)(ctx->launches % (int64_t)ctx->ev_start.size());
  if (single) {
    pe.start = ctx->ev_start[slot];
    pe.stop = ctx->ev_stop[slot];
    return hipSuccess;
  }
  return hipEventRecord(ctx->ev_start[slot], ctx->stream);
}

hipError_t time_end(mtg_ctx* ctx) {
  if (ctx->ev_start.empty()) return hipSuccess;
  const size_t slot = (size_t)(ctx->launches % (int64_t)ctx->ev_start.size());
  mtg::PendingEvents& pe = mtg::pending_events();
  hipError_t e = hipSuccess;
  if (pe.start) {
    if (!pe.used) {  // nothing was launched (e.g. an empty batch): an empty interval
      e = hipEventRecord(pe.start, ctx->stream);
      if (e == hipSuccess) e = hipEventRecord(pe.stop, ctx->stream);
    }
    pe = mtg::PendingEvents{};
  } else {
    e = hipEventRecord(ctx->ev_stop[slot], ctx->stream);
  }
  if (e == hipSuccess) ctx->launches++;
  return e;
}

void destroy_events(mtg_ctx* ctx) {
  for (hipEvent_t e : ctx->ev_start) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->ev_stop) (void)hipEventDestroy(e);
  ctx->ev_start.clear();
  ctx->ev_stop.clear();
  ctx->launches = 0;
}

hipError_t create_events(mtg_ctx* ctx, int ring) {
  destroy_events(ctx);
  for (int i = 0; i < ring; ++i) {
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    if (e != hipSuccess) {
      if (a) (void)hipEventDestroy(a);
      return e;
    }
    ctx->ev_start.push_back(a);
    ctx->ev_stop.push_back(b);
  }
  return hipSuccess;
}

// The argument checks that several entries make.  Each returns MTG_OK or the entry's return code with
// mtg_last_error set; an entry calls them in the order it reports its errors.
int check_order(mtg_ctx* ctx, int N) {
  if (N < 2 || N > 12 || (N % 2)) return set_error(ctx, MTG_ERR_UNSUPPORTED_N, "N must be even and in [2, 12]");
  return MTG_OK;
}

int check_dims(mtg_ctx* ctx, int D, int K, int64_t batch) {
  if (K < 1 || D < 1 || batch < 0) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need K >= 1, D >= 1, batch >= 0");
  return MTG_OK;
}

// the collision term's shape, grid and parameters; missing: the text for an absent grid or params
int check_collision(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const mtg_sdf_grid* grid,
                    const mtg_collision_params* params, const char* missing = "grid and params are required") {
  if (N < 6 || N > 12 || (N % 2)) return set_error(ctx, MTG_ERR_UNSUPPORTED_N, "N must be 6, 8, 10 or 12");
  if (D != 3) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "the collision term needs D == 3");
  if (K < 1 || batch < 0) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need K >= 1, batch >= 0");
  if (!grid || !params) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, missing);
  if (!(params->coll_check_time_increment > 0.0) || !(params->map_resolution >= 0.0) || !(grid->resolution > 0.0) ||
      grid->nx < 1 || grid->ny < 1 || grid->nz < 1)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                     "need coll_check_time_increment > 0, map_resolution >= 0, grid resolution > 0, grid dimensions >= 1");
  return MTG_OK;
}

// the soft-constraint parameters; count_text: the text for absent params or n_constraints out of [1, 8]
int check_soft_params(mtg_ctx* ctx, int N, const mtg_soft_constraint_params* p, const char* count_text) {
  if (!p || p->n_constraints < 1 || p->n_constraints > 8) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, count_text);
  const int kmax = N - 2 < 4 ? N - 2 : 4;
  for (int c = 0; c < p->n_constraints; ++c)
    if (p->derivative[c] < 0 || p->derivative[c] > kmax || !(p->limit[c] > 0.0))
      return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "need 0 <= derivative <= min(4, N - 2) and limit > 0");
  return MTG_OK;
}

int check_shape(mtg_ctx* ctx, int N, int D, int K, int r, int64_t batch) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  int rc = check_order(ctx, N);
  if (rc != MTG_OK) return rc;
  if (r < 0 || r > N / 2 - 1)
    return set_error(ctx, MTG_ERR_BAD_DERIVATIVE, "derivative_to_optimize must be in [0, N/2-1]");
  rc = check_dims(ctx, D, K, batch);
  if (rc != MTG_OK) return rc;
  int lg, tpb;
  size_t lds;
  if (!mtg::solve_geometry(N, D, K, &lg, &lds, &tpb))
    return set_error(ctx, MTG_ERR_TOO_LARGE, "per-trajectory working set exceeds LDS (reduce K or D)");
  return MTG_OK;
}

// MTG_HOST_WAIT=block: the pipeline's D2H thread sleeps on its chunk events (hipEventBlockingSync)
// instead of spinning on them (the runtime's default).  For measuring the host work of several
// concurrent pipelines (scripts/multi_host_cost.py): spinning waits make every waiting thread count
// as a busy core.  Read once per process.
bool host_wait_blocking() {
  static const bool b = [] {
    const char* v = getenv("MTG_HOST_WAIT");
    return v && strcmp(v, "block") == 0;
  }();
  return b;
}

hipError_t ensure_pipe(mtg_ctx* ctx) {
  if (ctx->pipe_start) return hipSuccess;
  const unsigned done_flags = hipEventDisableTiming | (host_wait_blocking() ? hipEventBlockingSync : 0u);
  for (auto& s : ctx->pipe) {
    hipError_t e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.in_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.k_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, done_flags);
    if (e != hipSuccess) return e;
  }
  hipError_t e = hipStreamCreateWithFlags(&ctx->pipe_h2d, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->pipe_d2h, hipStreamNonBlocking);
  if (e != hipSuccess) return e;
  return hipEventCreateWithFlags(&ctx->pipe_start, hipEventDisableTiming);
}

void destroy_pipe(mtg_ctx* ctx) {
  for (hipStream_t* q : {&ctx->pipe_h2d, &ctx->pipe_d2h}) {
    if (*q) (void)hipStreamSynchronize(*q);
  }
  for (auto& s : ctx->pipe) {
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.dev) (void)hipFree(s.dev);
    for (hipEvent_t ev : {s.in_done, s.k_done, s.done})
      if (ev) (void)hipEventDestroy(ev);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    s = mtg_ctx::PipeSlot{};
  }
  for (hipStream_t* q : {&ctx->pipe_h2d, &ctx->pipe_d2h}) {
    if (*q) (void)hipStreamDestroy(*q);
    *q = nullptr;
  }
  if (ctx->pipe_start) (void)hipEventDestroy(ctx->pipe_start);
  ctx->pipe_start = nullptr;
}

// The CPUs of the device's NUMA node that this process may run on (sysfs: the PCI device's numa_node
// and the node's cpulist), or nullptr when unknown, empty, or MTG_NO_NUMA_BIND is set.
const cpu_set_t* gpu_node_cpus(int device) {
  constexpr int kDevs = 64;
  static std::mutex mu;
  static cpu_set_t sets[kDevs];
  static bool known[kDevs] = {};
  if (device < 0 || device >= kDevs) return nullptr;
  std::lock_guard<std::mutex> g(mu);
  if (known[device]) return CPU_COUNT(&sets[device]) ? &sets[device] : nullptr;
  cpu_set_t& set = sets[device];
  CPU_ZERO(&set);
  char bus[64] = {0};
  const char* off = getenv("MTG_NO_NUMA_BIND");
  if (!(off && *off && *off != '0') && hipDeviceGetPCIBusId(bus, sizeof(bus), device) == hipSuccess) {
    for (char* c = bus; *c; ++c) *c = (char)tolower(*c);
    char path[160];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    int node = -1;
    if (FILE* f = fopen(path, "r")) {
      if (fscanf(f, "%d", &node) != 1) node = -1;
      fclose(f);
    }
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (node >= 0 && sched_getaffinity(0, sizeof(allowed), &allowed) == 0) {
      snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
      if (FILE* f = fopen(path, "r")) {
        int a = 0, b = 0;
        char sep = 0;
        while (fscanf(f, "%d", &a) == 1) {
          b = a;
          if (fscanf(f, "%c", &sep) == 1 && sep == '-') {
            if (fscanf(f, "%d", &b) != 1) b = a;
            if (fscanf(f, "%c", &sep) != 1) sep = 0;
          }
          for (int c = a; c <= b && c < CPU_SETSIZE; ++c)
            if (CPU_ISSET(c, &allowed)) CPU_SET(c, &set);
          if (sep != ',') break;
        }
        fclose(f);
      }
    }
  }
  known[device] = true;
  return CPU_COUNT(&set) ? &set : nullptr;
}

// host-pointer solves above this size go through the chunked pipeline
constexpr size_t kPipelineMinBytes = 8u << 20;
// returned by run_solve_pipelined when it could not start its D2H thread (nothing was issued)
constexpr int kPipelineUnavailable = 1;

// Host-pointer batch solve as a pipeline of chunks (the reference's equivalent is a
// loop of single solves, src/polynomial_timing_evaluation.cpp:119-126).  Each of kPipeSlots slots
// has its own kernel stream and device buffers.  This thread issues, per chunk, the H2D copies (on
// the context's one H2D stream) and the kernel (on the slot's stream, after the copies); a second
// host thread issues the chunk's D2H copies (on the one D2H stream, after the kernel) and retires
// it.  So the H2D of chunk c+1 runs on one DMA direction while the D2H of chunk c runs on the other
// (PCIe is full duplex: ~57 GB/s each way on MI355X, 97 GB/s both, scripts/pcie_bw.py), whether the
// caller's arrays are pinned (asynchronous copies) or pageable (the runtime's own staging, which
// blocks the issuing thread -- hence two threads).  One stream per copy direction: with the copies
// on the four slot streams, a pinned caller's copies of both directions were spread over the
// runtime's copy queues and the call ran in two modes (config 2, B = 125000: 7.0 or ~10-13 ms per
// call, median 9.8; pageable 6.6 ms).  A slot is reused only after its previous chunk's D2H completed.
int run_solve_pipelined(mtg_ctx* ctx, int N, int D, int K, int r, int64_t batch, const double* values,
                        const uint8_t* mask, const double* times, double* coeffs, double* free_out,
                        int32_t* n_free_out, double* cost_out, int32_t* status, unsigned kflags) {
  constexpr int S = mtg_ctx::kPipeSlots;
  const int V = K + 1, h = N / 2;
  // per-trajectory bytes of each array
  const size_t s_vals = sizeof(double) * (size_t)V * h * D, s_mask = (size_t)V, s_times = sizeof(double) * K;
  const size_t s_coef = coeffs ? sizeof(double) * (size_t)K * D * N : 0;
  const size_t s_free = free_out ? sizeof(double) * D * V * h : 0;
  const size_t s_nfree = n_free_out ? sizeof(int32_t) : 0, s_cost = cost_out ? sizeof(double) : 0;
  const size_t s_status = status ? sizeof(int32_t) : 0;
  const size_t per_traj = s_vals + s_mask + s_times + s_coef + s_free + s_nfree + s_cost + s_status;
  // a quarter of the batch per chunk (the pipeline fills and drains in a quarter of the run), at
  // most ~32 MB of traffic per chunk (per-chunk issue costs stay below ~5%)
  int64_t chunk = std::min<int64_t>((batch + 3) / 4, (int64_t)((32u << 20) / per_traj));
  chunk = (std::max<int64_t>(chunk, 1024) + 63) / 64 * 64;
  const int64_t n_chunks = (batch + chunk - 1) / chunk;
  size_t off = 0;  // one slot's device layout, 256-B aligned sub-buffers
  const size_t o_vals = off; off = align_up(off + s_vals * chunk);
  const size_t o_mask = off; off = align_up(off + s_mask * chunk);
  const size_t o_times = off; off = align_up(off + s_times * chunk);
  const size_t o_coef = off; off = align_up(off + s_coef * chunk);
  const size_t o_free = off; off = align_up(off + s_free * chunk);
  const size_t o_nfree = off; off = align_up(off + s_nfree * chunk);
  const size_t o_cost = off; off = align_up(off + s_cost * chunk);
  const size_t o_status = off; off = align_up(off + s_status * chunk);
  // the long-chain DL kernel's workspace, per slot (the slots' kernels may run at once)
  const unsigned ksel = kflags & (MTG_FLAG_GENERAL_KERNEL | MTG_FLAG_DL_KERNEL | MTG_FLAG_COLUMN_KERNEL);
  const size_t s_work = mtg::solve_kernel(N, D, K, ksel, r, chunk) == MTG_KERNEL_DLX
                            ? mtg::dlx_workspace_bytes(N, D, K, chunk) : 0;
  const size_t o_work = off; off = align_up(off + s_work);
  MTG_HIP_TRY(ctx, ensure_pipe(ctx));
  for (auto& s : ctx->pipe) MTG_HIP_TRY(ctx, ensure(&s.dev, &s.dev_bytes, off));

  std::mutex m;
  std::condition_variable cv;
  int64_t launched = 0, retired = 0;  // chunks whose kernel is queued / whose outputs have landed
  hipError_t err = hipSuccess;
  const char* err_what = "";
  auto fail = [&](hipError_t e, const char* what) {
    std::lock_guard<std::mutex> g(m);
    if (err == hipSuccess) err = e, err_what = what;
    cv.notify_all();
  };
  // D2H issuer: chunk c's outputs into the caller's arrays, on the chunk's slot stream (ordered after
  // its kernel), then wait for them and retire the chunk
  auto d2h_body = [&] {
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(e, "hipSetDevice");
    for (int64_t c = 0; c < n_chunks; ++c) {
      {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return launched > c || err != hipSuccess; });
        if (err != hipSuccess) return;
      }
      mtg_ctx::PipeSlot& s = ctx->pipe[c % S];
      const int64_t b0 = c * chunk, nb = std::min<int64_t>(chunk, batch - b0);
      const char* dp = static_cast<const char*>(s.dev);
      auto copy = [&](void* user, size_t o, size_t sz) -> hipError_t {
        return sz ? hipMemcpyAsync((char*)user + b0 * sz, dp + o, nb * sz, hipMemcpyDeviceToHost, ctx->pipe_d2h)
                  : hipSuccess;
      };
      e = hipStreamWaitEvent(ctx->pipe_d2h, s.k_done, 0);
      if (e == hipSuccess) e = copy(coeffs, o_coef, s_coef);
      if (e == hipSuccess) e = copy(free_out, o_free, s_free);
      if (e == hipSuccess) e = copy(n_free_out, o_nfree, s_nfree);
      if (e == hipSuccess) e = copy(cost_out, o_cost, s_cost);
      if (e == hipSuccess) e = copy(status, o_status, s_status);
      if (e == hipSuccess) e = hipEventRecord(s.done, ctx->pipe_d2h);
      // retire the previous chunk (its copies queued before this one's, so the DMA engine never
      // idles between chunks while this thread waits), and the last one at the end
      if (e == hipSuccess && c > 0) e = hipEventSynchronize(ctx->pipe[(c - 1) % S].done);
      if (e == hipSuccess && c + 1 == n_chunks) e = hipEventSynchronize(s.done);
      if (e != hipSuccess) return fail(e, "pipelined D2H");
      std::lock_guard<std::mutex> g(m);
      retired = c + 1 == n_chunks ? n_chunks : c;
      cv.notify_all();
    }
  };
  if (!ctx->d2h_worker.start(gpu_node_cpus(ctx->device)))
    return kPipelineUnavailable;  // no thread (std::system_error): nothing was issued, the caller stages
  ctx->d2h_worker.post(d2h_body);
  {
    // the pipeline's whole span (every chunk's H2D, kernel and D2H) is this call's timed interval;
    // the slot streams start after whatever the caller queued on the context's stream
    hipError_t e = time_begin(ctx, false);
    if (e == hipSuccess) e = hipEventRecord(ctx->pipe_start, ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->pipe_h2d, ctx->pipe_start, 0);
    if (e != hipSuccess) fail(e, "pipeline start");
  }
  // H2D + kernel issuer (this thread)
  for (int64_t c = 0; c < n_chunks; ++c) {
    {
      std::unique_lock<std::mutex> l(m);  // the slot's previous chunk must have landed
      cv.wait(l, [&] { return retired >= c - S + 1 || err != hipSuccess; });
      if (err != hipSuccess) break;
    }
    mtg_ctx::PipeSlot& s = ctx->pipe[c % S];
    const int64_t b0 = c * chunk, nb = std::min<int64_t>(chunk, batch - b0);
    char* dp = static_cast<char*>(s.dev);
    hipStream_t up = ctx->pipe_h2d;
    hipError_t e = hipMemcpyAsync(dp + o_vals, (const char*)values + b0 * s_vals, nb * s_vals,
                                  hipMemcpyHostToDevice, up);
    if (e == hipSuccess)
      e = hipMemcpyAsync(dp + o_mask, (const char*)mask + b0 * s_mask, nb * s_mask, hipMemcpyHostToDevice, up);
    if (e == hipSuccess)
      e = hipMemcpyAsync(dp + o_times, (const char*)times + b0 * s_times, nb * s_times, hipMemcpyHostToDevice, up);
    if (e == hipSuccess) e = hipEventRecord(s.in_done, up);
    if (e == hipSuccess) e = hipStreamWaitEvent(s.stream, s.in_done, 0);
    if (e == hipSuccess && free_out) e = hipMemsetAsync(dp + o_free, 0, nb * s_free, s.stream);
    if (e == hipSuccess) {
      mtg::SolveArgs a{};
      a.B = nb;
      a.K = K;
      a.D = D;
      a.r = r;
      a.n_cand = 1;
      a.values = reinterpret_cast<const double*>(dp + o_vals);
      a.mask = reinterpret_cast<const uint8_t*>(dp + o_mask);
      a.times = reinterpret_cast<const double*>(dp + o_times);
      a.coeffs = coeffs ? reinterpret_cast<double*>(dp + o_coef) : nullptr;
      a.free_out = free_out ? reinterpret_cast<double*>(dp + o_free) : nullptr;
      a.n_free_out = n_free_out ? reinterpret_cast<int32_t*>(dp + o_nfree) : nullptr;
      a.cost_out = cost_out ? reinterpret_cast<double*>(dp + o_cost) : nullptr;
      a.status = status ? reinterpret_cast<int32_t*>(dp + o_status) : nullptr;
      a.work = s_work ? reinterpret_cast<double*>(dp + o_work) : nullptr;
      a.work_bytes = (int64_t)s_work;
      e = mtg::launch_solve(N, a, s.stream, kflags);
    }
    if (e == hipSuccess) e = hipEventRecord(s.k_done, s.stream);
    if (e != hipSuccess) {
      fail(e, "pipelined H2D / launch");
      break;
    }
    std::lock_guard<std::mutex> g(m);
    launched = c + 1;
    cv.notify_all();
  }
  ctx->d2h_worker.wait();
  // nothing may still read or write the caller's arrays
  (void)hipStreamSynchronize(ctx->pipe_h2d);
  for (auto& s : ctx->pipe) (void)hipStreamSynchronize(s.stream);
  (void)hipStreamSynchronize(ctx->pipe_d2h);
  if (err != hipSuccess) return set_hip_error(ctx, err, err_what);
  // close the timed interval after the last D2H (every D2H is on pipe_d2h, in chunk order)
  MTG_HIP_TRY(ctx, hipEventRecord(ctx->pipe[(n_chunks - 1) % S].done, ctx->pipe_d2h));
  MTG_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->pipe[(n_chunks - 1) % S].done, 0));
  MTG_HIP_TRY(ctx, time_end(ctx));
  MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MTG_OK;
}

// Shared body of solve / time-sweep: stage host buffers if needed, launch, copy back.
int run_solve(mtg_ctx* ctx, int N, int D, int K, int r, int64_t batch, const double* values,
              const uint8_t* mask, const double* times, double* coeffs, double* free_out,
              int32_t* n_free_out, double* cost_out, int32_t* status, int n_cand,
              const double* scales, unsigned flags) {
  const int V = K + 1, h = N / 2;
  const int64_t pairs = batch * n_cand;
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // (a time sweep passes scales, also with one candidate: it takes the single-stream path, which stages them)
  if (!(flags & (MTG_FLAG_DEVICE_PTRS | MTG_FLAG_SPLIT_KERNELS)) && n_cand == 1 && !scales &&
      (size_t)batch * (sizeof(double) * ((size_t)V * h * D + K + (size_t)K * D * N) + V) > kPipelineMinBytes) {
    // the chunks run the kernel the whole batch would (the default is the same at every batch size;
    // the explicit flag keeps it so)
    const unsigned kf = flags & (MTG_FLAG_GENERAL_KERNEL |
                                 MTG_FLAG_DL_KERNEL | MTG_FLAG_COLUMN_KERNEL);
    const int kk = mtg::solve_kernel(N, D, K, kf, r, batch);
    const unsigned pin = (kk == MTG_KERNEL_DL || kk == MTG_KERNEL_DLX) ? MTG_FLAG_DL_KERNEL : MTG_FLAG_COLUMN_KERNEL;
    const int rc = run_solve_pipelined(ctx, N, D, K, r, batch, values, mask, times, coeffs, free_out, n_free_out,
                                       cost_out, status, kf | pin);
    if (rc != kPipelineUnavailable) return rc;
  }
  mtg::SolveArgs a{};
  a.B = pairs;
  a.K = K;
  a.D = D;
  a.r = r;
  a.n_cand = n_cand;
  const bool dev = flags & MTG_FLAG_DEVICE_PTRS;
  const size_t b_vals = sizeof(double) * (size_t)batch * V * h * D;
  const size_t b_mask = sizeof(uint8_t) * (size_t)batch * V;
  const size_t b_times = sizeof(double) * (size_t)batch * K;
  const size_t b_scales = scales ? sizeof(double) * (size_t)n_cand : 0;
  const size_t b_coeffs = coeffs ? sizeof(double) * (size_t)pairs * K * D * N : 0;
  const size_t b_free = free_out ? sizeof(double) * (size_t)pairs * D * V * h : 0;
  const size_t b_nfree = n_free_out ? sizeof(int32_t) * (size_t)pairs : 0;
  const size_t b_cost = cost_out ? sizeof(double) * (size_t)pairs : 0;
  const size_t b_status = status ? sizeof(int32_t) * (size_t)pairs : 0;
  char* base = nullptr;
  size_t o_vals = 0, o_mask = 0, o_times = 0, o_scales = 0, o_coeffs = 0, o_free = 0, o_nfree = 0,
         o_cost = 0, o_status = 0, out_end = 0;
  bool pin = false;
  if (dev) {
    a.values = values;
    a.mask = mask;
    a.times = times;
    a.scales = scales;
    a.coeffs = coeffs;
    a.free_out = free_out;
    a.n_free_out = n_free_out;
    a.cost_out = cost_out;
    a.status = status;
  } else {
    size_t off = 0;
    o_vals = off; off = align_up(off + b_vals);
    o_mask = off; off = align_up(off + b_mask);
    o_times = off; off = align_up(off + b_times);
    o_scales = off; off = align_up(off + b_scales);
    o_coeffs = off; off = align_up(off + b_coeffs);
    o_free = off; off = align_up(off + b_free);
    o_nfree = off; off = align_up(off + b_nfree);
    o_cost = off; off = align_up(off + b_cost);
    o_status = off; off = align_up(off + b_status);
    MTG_HIP_TRY(ctx, ensure(&ctx->staging, &ctx->staging_bytes, std::max<size_t>(off, 256)));
    base = static_cast<char*>(ctx->staging);
    pin = off <= kPinnedMax;
    if (pin) {
      // small call (a drop-in PolynomialOptimization::solveLinear): pack the inputs into a pinned
      // mirror of the staging layout and move them with ONE DMA each way, instead of one pageable
      // copy per array (each of which the runtime bounces through its own pinned buffer)
      if (ctx->pinned_bytes < off) {
        if (ctx->pinned) MTG_HIP_TRY(ctx, hipHostFree(ctx->pinned));
        ctx->pinned = nullptr;
        ctx->pinned_bytes = 0;
        MTG_HIP_TRY(ctx, hipHostMalloc(&ctx->pinned, kPinnedMax, hipHostMallocDefault));
        ctx->pinned_bytes = kPinnedMax;
      }
      char* hp = static_cast<char*>(ctx->pinned);
      std::memcpy(hp + o_vals, values, b_vals);
      std::memcpy(hp + o_mask, mask, b_mask);
      std::memcpy(hp + o_times, times, b_times);
      if (scales) std::memcpy(hp + o_scales, scales, b_scales);
      MTG_HIP_TRY(ctx, hipMemcpyAsync(base, hp, o_coeffs, hipMemcpyHostToDevice, ctx->stream));
    } else {
      MTG_HIP_TRY(ctx, hipMemcpyAsync(base + o_vals, values, b_vals, hipMemcpyHostToDevice, ctx->stream));
      MTG_HIP_TRY(ctx, hipMemcpyAsync(base + o_mask, mask, b_mask, hipMemcpyHostToDevice, ctx->stream));
      MTG_HIP_TRY(ctx, hipMemcpyAsync(base + o_times, times, b_times, hipMemcpyHostToDevice, ctx->stream));
      if (scales)
        MTG_HIP_TRY(ctx, hipMemcpyAsync(base + o_scales, scales, b_scales, hipMemcpyHostToDevice, ctx->stream));
    }
    out_end = off;
    a.values = reinterpret_cast<const double*>(base + o_vals);
    a.mask = reinterpret_cast<const uint8_t*>(base + o_mask);
    a.times = reinterpret_cast<const double*>(base + o_times);
    a.scales = scales ? reinterpret_cast<const double*>(base + o_scales) : nullptr;
    a.coeffs = coeffs ? reinterpret_cast<double*>(base + o_coeffs) : nullptr;
    a.free_out = free_out ? reinterpret_cast<double*>(base + o_free) : nullptr;
    a.n_free_out = n_free_out ? reinterpret_cast<int32_t*>(base + o_nfree) : nullptr;
    a.cost_out = cost_out ? reinterpret_cast<double*>(base + o_cost) : nullptr;
    a.status = status ? reinterpret_cast<int32_t*>(base + o_status) : nullptr;
  }
  // From here on a failure must not return while a DMA may still read ctx->pinned (the next call
  // would overwrite it): the pinned path drains the stream before reporting any error.
  struct PinnedDrain {
    mtg_ctx* ctx;
    bool armed;
    ~PinnedDrain() {
      if (armed) (void)hipStreamSynchronize(ctx->stream);
    }
  } drain{ctx, pin};
  if (free_out && b_free) {
    // entries beyond n_free are left zero
    MTG_HIP_TRY(ctx, hipMemsetAsync(const_cast<double*>(a.free_out), 0, b_free, ctx->stream));
  }
  const unsigned ksel = flags & (MTG_FLAG_GENERAL_KERNEL | MTG_FLAG_DL_KERNEL | MTG_FLAG_COLUMN_KERNEL);
  const bool dlx = !(flags & MTG_FLAG_SPLIT_KERNELS) && mtg::solve_kernel(N, D, K, ksel, r, pairs) == MTG_KERNEL_DLX;
  if (dlx) {  // the long-chain DL kernel's workspace (and two launches: the timed region spans both)
    const size_t wb = mtg::dlx_workspace_bytes(N, D, K, pairs);
    MTG_HIP_TRY(ctx, ensure(&ctx->workspace, &ctx->workspace_bytes, std::max<size_t>(wb, 256)));
    a.work = static_cast<double*>(ctx->workspace);
    a.work_bytes = (int64_t)ctx->workspace_bytes;
  }
  MTG_HIP_TRY(ctx, time_begin(ctx, !(flags & MTG_FLAG_SPLIT_KERNELS) && !dlx));
  if (flags & MTG_FLAG_SPLIT_KERNELS) {
    const size_t ws = mtg::split_workspace_bytes(N, D, K, pairs);
    MTG_HIP_TRY(ctx, ensure(&ctx->workspace, &ctx->workspace_bytes, std::max<size_t>(ws, 256)));
    MTG_HIP_TRY(ctx, mtg::launch_solve_split(N, a, ctx->workspace, ctx->stream));
  } else {
    MTG_HIP_TRY(ctx, mtg::launch_solve(N, a, ctx->stream, ksel));
  }
  MTG_HIP_TRY(ctx, time_end(ctx));
  if (pin) {
    char* hp = static_cast<char*>(ctx->pinned);
    MTG_HIP_TRY(ctx, hipMemcpyAsync(hp + o_coeffs, base + o_coeffs, out_end - o_coeffs, hipMemcpyDeviceToHost,
                                    ctx->stream));
    MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (coeffs) std::memcpy(coeffs, hp + o_coeffs, b_coeffs);
    if (free_out) std::memcpy(free_out, hp + o_free, b_free);
    if (n_free_out) std::memcpy(n_free_out, hp + o_nfree, b_nfree);
    if (cost_out) std::memcpy(cost_out, hp + o_cost, b_cost);
    if (status) std::memcpy(status, hp + o_status, b_status);
    drain.armed = false;
  } else if (!dev) {
    if (coeffs) MTG_HIP_TRY(ctx, hipMemcpyAsync(coeffs, base + o_coeffs, b_coeffs, hipMemcpyDeviceToHost, ctx->stream));
    if (free_out) MTG_HIP_TRY(ctx, hipMemcpyAsync(free_out, base + o_free, b_free, hipMemcpyDeviceToHost, ctx->stream));
    if (n_free_out) MTG_HIP_TRY(ctx, hipMemcpyAsync(n_free_out, base + o_nfree, b_nfree, hipMemcpyDeviceToHost, ctx->stream));
    if (cost_out) MTG_HIP_TRY(ctx, hipMemcpyAsync(cost_out, base + o_cost, b_cost, hipMemcpyDeviceToHost, ctx->stream));
    if (status) MTG_HIP_TRY(ctx, hipMemcpyAsync(status, base + o_status, b_status, hipMemcpyDeviceToHost, ctx->stream));
    MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  } else if (!(flags & MTG_FLAG_ASYNC)) {
    MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return MTG_OK;
}

// The call-level checks the three ragged entries share, in the order they are reported, and the plan.
// ctx may be NULL (mtg_solve_ragged_plan has none).  batch == 0 leaves an empty plan.
int ragged_check_and_plan(mtg_ctx* ctx, int N, int D, int r, int64_t batch, const int32_t* seg_count, unsigned flags,
                          mtg::RaggedPlan* plan) {
  int rc = check_order(ctx, N);
  if (rc != MTG_OK) return rc;
  if (r < 0 || r > N / 2 - 1)
    return set_error(ctx, MTG_ERR_BAD_DERIVATIVE, "derivative_to_optimize must be in [0, N/2-1]");
  if (D < 1 || batch < 0) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need D >= 1, batch >= 0");
  *plan = mtg::RaggedPlan{};
  plan->vo.assign(1, 0);
  plan->pvo.assign(1, 0);
  if (batch == 0) return MTG_OK;
  if (!seg_count) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "seg_count is required (a host array)");
  try {
    rc = mtg::ragged_plan(batch, seg_count, plan);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, MTG_ERR_OUT_OF_MEMORY, "ragged plan: out of host memory");
  }
  if (rc != MTG_OK) return set_error(ctx, rc, "every seg_count must be >= 1");
  for (const mtg::RaggedGroup& g : plan->groups) {
    rc = mtg_solve_kernel(N, D, g.K, r, flags);
    if (rc < 0) return set_error(ctx, rc, "a segment count of the batch is rejected by mtg_solve_kernel");
  }
  return MTG_OK;
}

// What the ragged entries share around ctx->ragged (the device copy of a call's small host-made
// arrays -- plan records, segment offsets -- and the packed arrays of gathered groups).
//
// An earlier ragged call may have run on another stream (mtg_set_stream): the next one reuses its
// buffer, so it waits for that call's last kernel first (ragged_wait_last), and records its own last
// kernel when it used the buffer (ragged_mark_last).
int ragged_wait_last(mtg_ctx* ctx) {
  if (ctx->ragged_done_pending) MTG_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ragged_done, 0));
  return MTG_OK;
}

int ragged_mark_last(mtg_ctx* ctx) {
  if (!ctx->ragged_done) MTG_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ragged_done, hipEventDisableTiming));
  MTG_HIP_TRY(ctx, hipEventRecord(ctx->ragged_done, ctx->stream));
  ctx->ragged_done_pending = true;
  return MTG_OK;
}

// The upload of `bytes` host-made bytes to dst (in ctx->ragged): fill(p) writes them into the pinned
// buffer whose turn it is, once the event behind that buffer's last upload has fired, and the copy is
// queued on ctx->stream.  The copy outlives an MTG_FLAG_ASYNC call, hence pinned memory the context
// owns; two buffers taken in turn, so that two such calls with different seg_count may follow each
// other without a synchronisation.
template <class Fill>
int ragged_upload(mtg_ctx* ctx, size_t bytes, void* dst, Fill fill) {
  mtg_ctx::RaggedHost& hb = ctx->ragged_host[ctx->ragged_turn];
  ctx->ragged_turn ^= 1;
  if (!hb.uploaded) MTG_HIP_TRY(ctx, hipEventCreateWithFlags(&hb.uploaded, hipEventDisableTiming));
  if (hb.pending) {
    MTG_HIP_TRY(ctx, hipEventSynchronize(hb.uploaded));
    hb.pending = false;
  }
  if (hb.bytes < bytes) {
    if (hb.p) MTG_HIP_TRY(ctx, hipHostFree(hb.p));
    hb.p = nullptr;
    hb.bytes = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 2, 4096);
    MTG_HIP_TRY(ctx, hipHostMalloc(&hb.p, want, hipHostMallocDefault));
    hb.bytes = want;
  }
  fill(hb.p);
  MTG_HIP_TRY(ctx, hipMemcpyAsync(dst, hb.p, bytes, hipMemcpyHostToDevice, ctx->stream));
  MTG_HIP_TRY(ctx, hipEventRecord(hb.uploaded, ctx->stream));
  hb.pending = true;
  return MTG_OK;
}

// one RaggedRec per gathered trajectory of the plan, to dst
int ragged_upload_records(mtg_ctx* ctx, const mtg::RaggedPlan& plan, void* dst) {
  const size_t nG = plan.members.size();
  return ragged_upload(ctx, sizeof(mtg::RaggedRec) * nG, dst, [&](void* p) {
    mtg::RaggedRec* recs = static_cast<mtg::RaggedRec*>(p);
    for (size_t j = 0; j < nG; ++j) {
      const int64_t b = plan.members[j];
      recs[j] = mtg::RaggedRec{plan.vo[(size_t)b], plan.pvo[j], b, (int32_t)(plan.vo[(size_t)b + 1] - plan.vo[(size_t)b] - 1), 0};
    }
  });
}

// The seg_count checks of mtg_evaluate_at_ragged_batch, after its checks on N, D, batch, M and the
// derivative arguments (the min / max entry gets the same two errors from its plan): seg_count present,
// every entry >= 1.  *k_max receives the largest and *so the segment offsets [batch + 1].  batch == 0:
// nothing is checked and *so stays empty.
int ragged_check_counts(mtg_ctx* ctx, int64_t batch, const int32_t* seg_count, int* k_max, std::vector<int64_t>* so) {
  *k_max = 0;
  if (batch == 0) return MTG_OK;
  if (!seg_count) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "seg_count is required (a host array)");
  so->assign((size_t)batch + 1, 0);
  for (int64_t b = 0; b < batch; ++b) {
    if (seg_count[b] < 1) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "every seg_count must be >= 1");
    *k_max = std::max<int>(*k_max, seg_count[b]);
    (*so)[(size_t)b + 1] = (*so)[(size_t)b] + seg_count[b];
  }
  return MTG_OK;
}

// Body of mtg_evaluate_at_ragged_batch: the segment offsets to ctx->ragged, then one
// launch of the ragged kernels on the caller's CSR arrays; nothing is copied on the device.
int run_evaluate_at_ragged(mtg_ctx* ctx, int N, int D, int k_max, const std::vector<int64_t>& so, const double* coeffs,
                           const double* times, const double* t_query, int64_t t_stride, int64_t M, int k0, int nd,
                           double* out, uint8_t* in_range_out, int32_t* status, unsigned flags) {
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nB = so.size() - 1, nM = (size_t)M, totS = (size_t)so.back();
  const double *d_coef, *d_times, *d_tq;
  double* d_out;
  uint8_t* d_in;
  int32_t* d_status;
  Staged st(ctx, flags);
  st.in(&d_coef, coeffs, sizeof(double) * totS * D * N);
  st.in(&d_times, times, sizeof(double) * totS);
  st.in(&d_tq, t_query, sizeof(double) * (t_stride ? (nB - 1) * (size_t)t_stride + nM : nM));
  st.out(&d_out, out, sizeof(double) * nB * nM * nd * D);
  st.out(&d_in, in_range_out, nB * nM);
  st.out(&d_status, status, sizeof(int32_t) * nB);
  if (int rc = ragged_wait_last(ctx)) return rc;
  if (int rc = st.upload()) return rc;
  const size_t b_so = sizeof(int64_t) * so.size();
  MTG_HIP_TRY(ctx, ensure(&ctx->ragged, &ctx->ragged_bytes, align_up(b_so)));
  if (int rc = ragged_upload(ctx, b_so, ctx->ragged, [&](void* p) { std::memcpy(p, so.data(), b_so); })) return rc;
  MTG_HIP_TRY(ctx, time_begin(ctx));
  MTG_HIP_TRY(ctx, mtg::launch_evaluate_at_ragged(N, D, k_max, (int64_t)nB, static_cast<const int64_t*>(ctx->ragged),
                                                  d_coef, d_times, d_tq, t_stride, M, k0, nd, d_out, d_in, d_status,
                                                  ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  if (int rc = ragged_mark_last(ctx)) return rc;
  return st.finish();
}

// Body of mtg_min_max_magnitude_ragged_batch.  The extrema kernel's bits depend on
// the block geometry its launcher derives from K, so every K-group goes through the unchanged uniform
// launcher: in place on slices of the caller's arrays (the kernel reads coeffs and times as doubles and
// writes whole mtg_extremum structs: 8-byte alignment is all a slice needs), or on packed copies of
// the gathered groups' coefficients and times, whose results one kernel then moves to minimum[b] and
// maximum[b].  Upload, gather, one launch per group in ascending K, scatter: one stream, no host
// synchronisation in between.
int run_min_max_ragged(mtg_ctx* ctx, int N, int D, const mtg::RaggedPlan& plan, const double* coeffs, const double* times,
                       int derivative, uint32_t dims, mtg_extremum* minimum, mtg_extremum* maximum, unsigned flags) {
  const size_t DN = (size_t)D * N;
  const size_t nB = plan.vo.size() - 1, totS = (size_t)plan.total_segments();
  const size_t nG = plan.members.size(), gS = (size_t)plan.pvo.back() - nG;
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const double *d_coef, *d_times;
  mtg_extremum *d_min, *d_max;
  Staged st(ctx, flags);
  st.in(&d_coef, coeffs, sizeof(double) * totS * DN);
  st.in(&d_times, times, sizeof(double) * totS);
  st.out(&d_min, minimum, sizeof(mtg_extremum) * nB);
  st.out(&d_max, maximum, sizeof(mtg_extremum) * nB);
  if (int rc = ragged_wait_last(ctx)) return rc;
  if (int rc = st.upload()) return rc;
  mtg::RaggedCoeffArgs ca{};
  if (nG) {
    size_t off = 0;
    const size_t o_recs = off; off = align_up(off + sizeof(mtg::RaggedRec) * nG);
    const size_t o_coef = off; off = align_up(off + sizeof(double) * gS * DN);
    const size_t o_times = off; off = align_up(off + sizeof(double) * gS);
    const size_t o_min = off; off = align_up(off + (d_min ? sizeof(mtg_extremum) * nG : 0));
    const size_t o_max = off; off = align_up(off + (d_max ? sizeof(mtg_extremum) * nG : 0));
    MTG_HIP_TRY(ctx, ensure(&ctx->ragged, &ctx->ragged_bytes, off));
    char* base = static_cast<char*>(ctx->ragged);
    if (int rc = ragged_upload_records(ctx, plan, base + o_recs)) return rc;
    ca.recs = reinterpret_cast<const mtg::RaggedRec*>(base + o_recs);
    ca.n = (int64_t)nG;
    ca.DN = (int)DN;
    ca.coeffs = d_coef;
    ca.times = d_times;
    ca.p_coeffs = reinterpret_cast<double*>(base + o_coef);
    ca.p_times = reinterpret_cast<double*>(base + o_times);
    ca.p_minimum = d_min ? reinterpret_cast<mtg_extremum*>(base + o_min) : nullptr;
    ca.p_maximum = d_max ? reinterpret_cast<mtg_extremum*>(base + o_max) : nullptr;
    ca.minimum = d_min;
    ca.maximum = d_max;
  }
  MTG_HIP_TRY(ctx, time_begin(ctx, false));
  if (nG) MTG_HIP_TRY(ctx, mtg::launch_ragged_gather_coeffs(ca, ctx->stream));
  for (const mtg::RaggedGroup& g : plan.groups) {
    // the group's arrays: slices of the CSR arrays at its first member, or of the packed arrays
    const int64_t s0 = g.in_place ? plan.so(g.first) : plan.pso(g.first);
    const double* gc = (g.in_place ? d_coef : ca.p_coeffs) + s0 * DN;
    const double* gt = (g.in_place ? d_times : ca.p_times) + s0;
    mtg_extremum* gmin = g.in_place ? d_min : ca.p_minimum;
    mtg_extremum* gmax = g.in_place ? d_max : ca.p_maximum;
    MTG_HIP_TRY(ctx, mtg::launch_min_max_magnitude(N, gc, gt, g.count, g.K, D, derivative, dims,
                                                   gmin ? gmin + g.first : nullptr, gmax ? gmax + g.first : nullptr,
                                                   ctx->stream));
  }
  if (nG) MTG_HIP_TRY(ctx, mtg::launch_ragged_scatter_extrema(ca, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  if (nG)
    if (int rc = ragged_mark_last(ctx)) return rc;
  return st.finish();
}

// Body of mtg_solve_linear_ragged_batch: the gathered groups' inputs into packed
// arrays (one kernel), one uniform solve launch per group in ascending K -- in place on slices of the
// CSR arrays, or on the packed arrays -- and the gathered groups' outputs back (one kernel); all on
// ctx->stream with no host synchronisation in between.
int run_solve_ragged(mtg_ctx* ctx, int N, int D, int r, const mtg::RaggedPlan& plan, const double* values,
                     const uint8_t* mask, const double* times, double* coeffs, double* free_out, int32_t* n_free_out,
                     double* cost_out, int32_t* status, unsigned flags) {
  const int h = N / 2;
  const size_t hD = (size_t)h * D, DN = (size_t)D * N;
  const int64_t batch = (int64_t)plan.vo.size() - 1;
  const size_t totV = (size_t)plan.total_vertices(), totS = (size_t)plan.total_segments();
  const size_t nG = plan.members.size(), gV = (size_t)plan.pvo.back(), gS = gV - nG;
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const double *d_vals, *d_times;
  const uint8_t* d_mask;
  double *d_coeffs, *d_free, *d_cost;
  int32_t *d_nfree, *d_status;
  const size_t b_free = sizeof(double) * totV * hD;
  Staged st(ctx, flags);
  st.in(&d_vals, values, sizeof(double) * totV * hD);
  st.in(&d_mask, mask, totV);
  st.in(&d_times, times, sizeof(double) * totS);
  st.out(&d_coeffs, coeffs, sizeof(double) * totS * DN);
  st.out(&d_free, free_out, b_free);
  st.out(&d_nfree, n_free_out, sizeof(int32_t) * (size_t)batch);
  st.out(&d_cost, cost_out, sizeof(double) * (size_t)batch);
  st.out(&d_status, status, sizeof(int32_t) * (size_t)batch);
  if (int rc = ragged_wait_last(ctx)) return rc;
  if (int rc = st.upload()) return rc;

  // the DLX / split workspace, sized once for the largest group that needs it, before the first
  // launch: growing it between launches would free memory a queued kernel uses
  const unsigned ksel = flags & (MTG_FLAG_GENERAL_KERNEL | MTG_FLAG_DL_KERNEL | MTG_FLAG_COLUMN_KERNEL);
  const bool split = flags & MTG_FLAG_SPLIT_KERNELS;
  size_t work = 0;
  for (const mtg::RaggedGroup& g : plan.groups) {
    if (split) work = std::max(work, mtg::split_workspace_bytes(N, D, g.K, g.count));
    else if (mtg::solve_kernel(N, D, g.K, ksel, r, g.count) == MTG_KERNEL_DLX)
      work = std::max(work, mtg::dlx_workspace_bytes(N, D, g.K, g.count));
  }
  if (work) MTG_HIP_TRY(ctx, ensure(&ctx->workspace, &ctx->workspace_bytes, std::max<size_t>(work, 256)));

  // the ragged buffer: the records, then the packed arrays of the gathered trajectories (only the
  // outputs the caller asked for), 256-B aligned each
  mtg::RaggedCopyArgs ca{};
  if (nG) {
    size_t off = 0;
    const size_t o_recs = off; off = align_up(off + sizeof(mtg::RaggedRec) * nG);
    const size_t o_vals = off; off = align_up(off + sizeof(double) * gV * hD);
    const size_t o_mask = off; off = align_up(off + gV);
    const size_t o_times = off; off = align_up(off + sizeof(double) * gS);
    const size_t o_coef = off; off = align_up(off + (d_coeffs ? sizeof(double) * gS * DN : 0));
    const size_t o_free = off; off = align_up(off + (d_free ? sizeof(double) * gV * hD : 0));
    const size_t o_nfree = off; off = align_up(off + (d_nfree ? sizeof(int32_t) * nG : 0));
    const size_t o_cost = off; off = align_up(off + (d_cost ? sizeof(double) * nG : 0));
    const size_t o_status = off; off = align_up(off + (d_status ? sizeof(int32_t) * nG : 0));
    MTG_HIP_TRY(ctx, ensure(&ctx->ragged, &ctx->ragged_bytes, off));
    char* base = static_cast<char*>(ctx->ragged);
    if (int rc = ragged_upload_records(ctx, plan, base + o_recs)) return rc;
    ca.recs = reinterpret_cast<const mtg::RaggedRec*>(base + o_recs);
    ca.n = (int64_t)nG;
    ca.hD = (int)hD;
    ca.DN = (int)DN;
    ca.values = d_vals;
    ca.mask = d_mask;
    ca.times = d_times;
    ca.coeffs = d_coeffs;
    ca.free = d_free;
    ca.cost = d_cost;
    ca.n_free = d_nfree;
    ca.status = d_status;
    ca.p_values = reinterpret_cast<double*>(base + o_vals);
    ca.p_mask = reinterpret_cast<uint8_t*>(base + o_mask);
    ca.p_times = reinterpret_cast<double*>(base + o_times);
    ca.p_coeffs = d_coeffs ? reinterpret_cast<double*>(base + o_coef) : nullptr;
    ca.p_free = d_free ? reinterpret_cast<double*>(base + o_free) : nullptr;
    ca.p_cost = d_cost ? reinterpret_cast<double*>(base + o_cost) : nullptr;
    ca.p_n_free = d_nfree ? reinterpret_cast<int32_t*>(base + o_nfree) : nullptr;
    ca.p_status = d_status ? reinterpret_cast<int32_t*>(base + o_status) : nullptr;
    // entries beyond n_free are left zero (the scatter copies whole blocks)
    if (d_free) MTG_HIP_TRY(ctx, hipMemsetAsync(base + o_free, 0, sizeof(double) * gV * hD, ctx->stream));
  }
  if (d_free && plan.n_in_place) MTG_HIP_TRY(ctx, hipMemsetAsync(d_free, 0, b_free, ctx->stream));

  MTG_HIP_TRY(ctx, time_begin(ctx, false));
  if (nG) MTG_HIP_TRY(ctx, mtg::launch_ragged_gather(ca, ctx->stream));
  for (const mtg::RaggedGroup& g : plan.groups) {
    // the group's arrays: slices of the CSR arrays at its first member, or of the packed arrays
    const int64_t v0 = g.in_place ? plan.vo[(size_t)g.first] : plan.pvo[(size_t)g.first];
    const int64_t s0 = v0 - g.first, t0 = g.first;
    mtg::SolveArgs a{};
    a.B = g.count;
    a.K = g.K;
    a.D = D;
    a.r = r;
    a.n_cand = 1;
    if (g.in_place) {
      a.values = d_vals + v0 * hD;
      a.mask = d_mask + v0;
      a.times = d_times + s0;
      a.coeffs = d_coeffs ? d_coeffs + s0 * DN : nullptr;
      a.free_out = d_free ? d_free + v0 * hD : nullptr;
      a.n_free_out = d_nfree ? d_nfree + t0 : nullptr;
      a.cost_out = d_cost ? d_cost + t0 : nullptr;
      a.status = d_status ? d_status + t0 : nullptr;
    } else {
      a.values = ca.p_values + v0 * hD;
      a.mask = ca.p_mask + v0;
      a.times = ca.p_times + s0;
      a.coeffs = ca.p_coeffs ? const_cast<double*>(ca.p_coeffs) + s0 * DN : nullptr;
      a.free_out = ca.p_free ? const_cast<double*>(ca.p_free) + v0 * hD : nullptr;
      a.n_free_out = ca.p_n_free ? const_cast<int32_t*>(ca.p_n_free) + t0 : nullptr;
      a.cost_out = ca.p_cost ? const_cast<double*>(ca.p_cost) + t0 : nullptr;
      a.status = ca.p_status ? const_cast<int32_t*>(ca.p_status) + t0 : nullptr;
    }
    if (split) {
      MTG_HIP_TRY(ctx, mtg::launch_solve_split(N, a, ctx->workspace, ctx->stream));
    } else {
      if (mtg::solve_kernel(N, D, g.K, ksel, r, g.count) == MTG_KERNEL_DLX) {
        a.work = static_cast<double*>(ctx->workspace);
        a.work_bytes = (int64_t)ctx->workspace_bytes;
      }
      MTG_HIP_TRY(ctx, mtg::launch_solve(N, a, ctx->stream, ksel));
    }
  }
  if (nG) MTG_HIP_TRY(ctx, mtg::launch_ragged_scatter(ca, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  if (nG)
    if (int rc = ragged_mark_last(ctx)) return rc;
  return st.finish();
}

}  // namespace

extern "C" {

int mtg_abi_version(void) { return MTG_ABI_VERSION; }

int mtg_solve_kernel(int N, int D, int K, int derivative_to_optimize, unsigned flags) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (derivative_to_optimize < 0 || derivative_to_optimize > N / 2 - 1) return MTG_ERR_BAD_DERIVATIVE;
  if (K < 1 || D < 1) return MTG_ERR_SIZE_MISMATCH;
  int lg, tpb;
  size_t lds;
  if (!mtg::solve_geometry(N, D, K, &lg, &lds, &tpb)) return MTG_ERR_TOO_LARGE;
  if (flags & MTG_FLAG_SPLIT_KERNELS) return MTG_KERNEL_SPLIT;
  return mtg::solve_kernel(N, D, K, flags, derivative_to_optimize);
}

int mtg_solve_kernel_batch(int N, int D, int K, int derivative_to_optimize, int64_t B, unsigned flags) {
  const int k = mtg_solve_kernel(N, D, K, derivative_to_optimize, flags);
  if (k < 0 || k == MTG_KERNEL_SPLIT || B < 0) return k;
  return mtg::solve_kernel(N, D, K, flags, derivative_to_optimize, B);
}

const char* mtg_status_string(int code) {
  switch (code) {
    case MTG_OK: return "ok";
    case MTG_ERR_INVALID_ARGUMENT: return "invalid argument";
    case MTG_ERR_UNSUPPORTED_N: return "unsupported N (even, 2..12)";
    case MTG_ERR_BAD_DERIVATIVE: return "derivative_to_optimize out of [0, N/2-1]";
    case MTG_ERR_SIZE_MISMATCH: return "size mismatch";
    case MTG_ERR_HIP: return "HIP runtime error";
    case MTG_ERR_NO_DEVICE: return "no HIP device";
    case MTG_ERR_OUT_OF_MEMORY: return "out of device memory";
    case MTG_ERR_TOO_LARGE: return "problem too large for the LDS-resident solver";
    default: return "unknown status";
  }
}

const char* mtg_last_error(mtg_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int mtg_device_count(int* count) {
  if (!count) return MTG_ERR_INVALID_ARGUMENT;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return e == hipErrorNoDevice ? MTG_ERR_NO_DEVICE : MTG_ERR_HIP;
  }
  *count = n;
  return MTG_OK;
}

int mtg_create(int device, mtg_ctx** out_ctx) {
  if (!out_ctx) return MTG_ERR_INVALID_ARGUMENT;
  *out_ctx = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return MTG_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return MTG_ERR_INVALID_ARGUMENT;
  mtg_ctx* ctx = new (std::nothrow) mtg_ctx();
  if (!ctx) return MTG_ERR_OUT_OF_MEMORY;
  ctx->device = device;
  hipError_t e = hipSetDevice(device);
  // (MTG_HOST_WAIT=block: every wait of the process's HIP runtime on this device sleeps, including
  // the runtime's own waits inside pageable copies; measurement only, see host_wait_blocking)
  if (e == hipSuccess && host_wait_blocking()) (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = create_events(ctx, 1);
  if (e != hipSuccess) {
    mtg_destroy(ctx);
    return MTG_ERR_HIP;
  }
  ctx->stream = ctx->own_stream;
  *out_ctx = ctx;
  return MTG_OK;
}

int mtg_destroy(mtg_ctx* ctx) {
  if (!ctx) return MTG_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->staging) (void)hipFree(ctx->staging);
  if (ctx->workspace) (void)hipFree(ctx->workspace);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->ragged_done) {  // (a ragged call may have run on a stream that is no longer the context's)
    if (ctx->ragged_done_pending) (void)hipEventSynchronize(ctx->ragged_done);
    (void)hipEventDestroy(ctx->ragged_done);
  }
  for (auto& hb : ctx->ragged_host) {
    if (hb.uploaded) (void)hipEventDestroy(hb.uploaded);
    if (hb.p) (void)hipHostFree(hb.p);
  }
  if (ctx->ragged) (void)hipFree(ctx->ragged);
  destroy_pipe(ctx);
  destroy_events(ctx);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
  return MTG_OK;
}

int mtg_set_stream(mtg_ctx* ctx, void* hip_stream) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(ctx->mu);
  ctx->stream = static_cast<hipStream_t>(hip_stream);  // NULL = the HIP null stream
  return MTG_OK;
}

int mtg_reset_stream(mtg_ctx* ctx) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(ctx->mu);
  ctx->stream = ctx->own_stream;
  return MTG_OK;
}

void* mtg_get_stream(mtg_ctx* ctx) { return ctx ? static_cast<void*>(ctx->stream) : nullptr; }

int mtg_synchronize(mtg_ctx* ctx) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MTG_OK;
}

int mtg_solve_linear_batch(mtg_ctx* ctx, int N, int D, int K, int derivative_to_optimize,
                           int64_t batch, const double* values, const uint8_t* fixed_mask,
                           const double* times, double* coeffs, double* free_out,
                           int32_t* n_free_out, double* cost_out, int32_t* status,
                           unsigned flags) {
  int rc = check_shape(ctx, N, D, K, derivative_to_optimize, batch);
  if (rc != MTG_OK) return rc;
  if (batch == 0) return MTG_OK;
  if (!values || !fixed_mask || !times)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "values, fixed_mask and times are required");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (ctx->inject_rc) {  // (diagnostics: mtg_debug_fail_next_solve)
    const int code = ctx->inject_rc;
    ctx->inject_rc = 0;
    return set_error(ctx, code, "injected fault (mtg_debug_fail_next_solve)");
  }
  return run_solve(ctx, N, D, K, derivative_to_optimize, batch, values, fixed_mask, times, coeffs,
                   free_out, n_free_out, cost_out, status, 1, nullptr, flags);
}

int mtg_solve_ragged_plan(int N, int D, int derivative_to_optimize, int64_t batch, const int32_t* seg_count,
                          unsigned flags, int64_t* n_groups, int64_t* n_in_place, int64_t* total_segments) {
  mtg::RaggedPlan plan;
  const int rc = ragged_check_and_plan(nullptr, N, D, derivative_to_optimize, batch, seg_count, flags, &plan);
  if (rc != MTG_OK) return rc;
  if (n_groups) *n_groups = (int64_t)plan.groups.size();
  if (n_in_place) *n_in_place = plan.n_in_place;
  if (total_segments) *total_segments = plan.total_segments();
  return MTG_OK;
}

int mtg_solve_linear_ragged_batch(mtg_ctx* ctx, int N, int D, int derivative_to_optimize, int64_t batch,
                                  const int32_t* seg_count, const double* values, const uint8_t* fixed_mask,
                                  const double* times, double* coeffs, double* free_out, int32_t* n_free_out,
                                  double* cost_out, int32_t* status, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  mtg::RaggedPlan plan;
  const int rc = ragged_check_and_plan(ctx, N, D, derivative_to_optimize, batch, seg_count, flags, &plan);
  if (rc != MTG_OK) return rc;
  if (batch == 0) return MTG_OK;
  if (!values || !fixed_mask || !times)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "values, fixed_mask and times are required");
  std::lock_guard<std::mutex> g(ctx->mu);
  try {
    return run_solve_ragged(ctx, N, D, derivative_to_optimize, plan, values, fixed_mask, times, coeffs, free_out,
                            n_free_out, cost_out, status, flags);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, MTG_ERR_OUT_OF_MEMORY, "ragged solve: out of host memory");
  }
}

int mtg_debug_fail_next_solve(mtg_ctx* ctx, int code) {
  if (!ctx || code >= 0) return MTG_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(ctx->mu);
  ctx->inject_rc = code;
  return MTG_OK;
}

int mtg_shard_range(int64_t batch, int n_shards, int shard, int64_t* begin, int64_t* end) {
  if (batch < 0 || n_shards < 1 || shard < 0 || shard >= n_shards || !begin || !end) return MTG_ERR_INVALID_ARGUMENT;
  const int64_t per = (batch + n_shards - 1) / n_shards;  // ceil(B / G), SURVEY.md 8(e)
  *begin = std::min<int64_t>(batch, (int64_t)shard * per);
  *end = std::min<int64_t>(batch, *begin + per);
  return MTG_OK;
}

int mtg_solve_linear_batch_multi(mtg_ctx* const* ctxs, int n_ctxs, int N, int D, int K, int derivative_to_optimize,
                                 int64_t batch, const double* values, const uint8_t* fixed_mask,
                                 const double* times, double* coeffs, double* free_out, int32_t* n_free_out,
                                 double* cost_out, int32_t* status, unsigned flags) {
  if (!ctxs || n_ctxs < 1) return MTG_ERR_INVALID_ARGUMENT;
  for (int g = 0; g < n_ctxs; ++g)
    if (!ctxs[g]) return MTG_ERR_INVALID_ARGUMENT;
  mtg_ctx* c0 = ctxs[0];
  if (flags & (MTG_FLAG_DEVICE_PTRS | MTG_FLAG_ASYNC))
    return set_error(c0, MTG_ERR_INVALID_ARGUMENT, "multi-device solves take host arrays and are synchronous");
  int rc = check_shape(c0, N, D, K, derivative_to_optimize, batch);
  if (rc != MTG_OK) return rc;
  if (batch == 0) return MTG_OK;
  if (!values || !fixed_mask || !times)
    return set_error(c0, MTG_ERR_INVALID_ARGUMENT, "values, fixed_mask and times are required");
  const int V = K + 1, h = N / 2;
  const size_t s_vals = (size_t)V * h * D, s_coef = (size_t)K * D * N, s_free = (size_t)D * V * h;
  std::vector<int> rcs(n_ctxs, MTG_OK);
  // every shard runs the kernel the whole batch would on one device (the default no longer depends on
  // the batch size -- the DL kernel for N = 10 / K = 10 and N = 12 / K = 20 at every size -- but the
  // flag keeps the choice explicit), so the result does not depend on the number of devices
  if (!(flags & MTG_FLAG_SPLIT_KERNELS))
  {
    const int kk = mtg::solve_kernel(N, D, K, flags, derivative_to_optimize, batch);
    flags |= (kk == MTG_KERNEL_DL || kk == MTG_KERNEL_DLX) ? MTG_FLAG_DL_KERNEL : MTG_FLAG_COLUMN_KERNEL;
  }
  auto shard = [&](int g) {
    int64_t b0 = 0, b1 = 0;
    mtg_shard_range(batch, n_ctxs, g, &b0, &b1);
    if (b1 <= b0) return;
    rcs[g] = mtg_solve_linear_batch(ctxs[g], N, D, K, derivative_to_optimize, b1 - b0, values + b0 * s_vals,
                                    fixed_mask + b0 * V, times + b0 * K, coeffs ? coeffs + b0 * s_coef : nullptr,
                                    free_out ? free_out + b0 * s_free : nullptr, n_free_out ? n_free_out + b0 : nullptr,
                                    cost_out ? cost_out + b0 : nullptr, status ? status + b0 : nullptr, flags);
  };
  // one host thread per context: each drives its device's staging or chunk pipeline and writes its
  // disjoint slice of the outputs (no collective); shard 0 runs on this thread
  std::vector<std::thread> pool;
  for (int g = 1; g < n_ctxs; ++g) {
    try {
      pool.emplace_back(shard, g);
    } catch (...) {  // no thread: solve this shard here instead
      shard(g);
    }
  }
  shard(0);
  for (auto& t : pool) t.join();
  for (int g = 0; g < n_ctxs; ++g) {
    if (rcs[g] == MTG_OK) continue;
    std::string what;
    {
      std::lock_guard<std::mutex> l(ctxs[g]->mu);
      what = ctxs[g]->last_error;
    }
    std::lock_guard<std::mutex> l(c0->mu);
    c0->last_error = "shard " + std::to_string(g) + " of " + std::to_string(n_ctxs) + ": " + what;
    return rcs[g];
  }
  return MTG_OK;
}

int mtg_time_sweep_batch(mtg_ctx* ctx, int N, int D, int K, int derivative_to_optimize,
                         int64_t batch, const double* values, const uint8_t* fixed_mask,
                         const double* times, int n_candidates, const double* scales,
                         double* cost_out, int32_t* status, unsigned flags) {
  int rc = check_shape(ctx, N, D, K, derivative_to_optimize, batch);
  if (rc != MTG_OK) return rc;
  if (n_candidates < 1) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "n_candidates must be >= 1");
  if (batch == 0) return MTG_OK;
  if (!values || !fixed_mask || !times || !scales || !cost_out)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "values, fixed_mask, times, scales, cost_out are required");
  std::lock_guard<std::mutex> g(ctx->mu);
  return run_solve(ctx, N, D, K, derivative_to_optimize, batch, values, fixed_mask, times, nullptr,
                   nullptr, nullptr, cost_out, status, n_candidates, scales,
                   flags);
}

int mtg_cost_at_times_batch(mtg_ctx* ctx, int N, int D, int K, int derivative_to_optimize,
                            int64_t batch, const double* vertex_values, const uint8_t* fixed_mask,
                            const double* times, int n_candidates, const double* scales,
                            double* cost_out, double* grad_out, unsigned flags) {
  int rc = check_shape(ctx, N, D, K, derivative_to_optimize, batch);
  if (rc != MTG_OK) return rc;
  if (n_candidates < 1) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "n_candidates must be >= 1");
  if (batch == 0) return MTG_OK;
  if (!vertex_values || !times || !scales || !cost_out || (grad_out && !fixed_mask))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                     "vertex_values, times, scales, cost_out are required; grad_out needs fixed_mask");
  if (mtg::cost_lds_bytes(N, D, K) > 64 * 1024)
    return set_error(ctx, MTG_ERR_TOO_LARGE, "per-trajectory cost tables exceed LDS (reduce K or D)");
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int V = K + 1, h = N / 2, C = n_candidates;
  const size_t nB = (size_t)batch, b_grad = sizeof(double) * nB * C * D * V * h;
  const double *d_vals, *d_times, *d_scales;
  const uint8_t* d_mask;
  double *d_cost, *d_grad;
  Staged st(ctx, flags);
  st.in(&d_vals, vertex_values, sizeof(double) * nB * V * h * D);
  st.in(&d_mask, fixed_mask, grad_out ? nB * V : 0);
  st.in(&d_times, times, sizeof(double) * nB * K);
  st.in(&d_scales, scales, sizeof(double) * (size_t)C * K);
  st.out(&d_cost, cost_out, sizeof(double) * nB * C);
  st.out(&d_grad, grad_out, b_grad);
  if (int rc = st.upload()) return rc;
  if (d_grad) MTG_HIP_TRY(ctx, hipMemsetAsync(d_grad, 0, b_grad, ctx->stream));
  MTG_HIP_TRY(ctx, time_begin(ctx));
  MTG_HIP_TRY(ctx, mtg::launch_cost_at_times(N, derivative_to_optimize, d_vals, d_mask, d_times, d_scales, d_cost,
                                             d_grad, batch, K, D, C, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  return st.finish();
}

int mtg_collision_cost_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* vertex_values,
                             const uint8_t* fixed_mask, const double* times, const mtg_sdf_grid* grid,
                             const mtg_collision_params* params, double* cost_out, double* grad_out,
                             uint8_t* collision_out, int32_t* n_evaluated_out, int32_t* status, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_collision(ctx, N, D, K, batch, grid, params)) return rc;
  if (batch == 0) return MTG_OK;
  if (!vertex_values || !times || !cost_out || !grid->distance || (grad_out && !fixed_mask))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                     "vertex_values, times, cost_out and grid->distance are required; grad_out needs fixed_mask");
  if (mtg::collision_lds_bytes(N, K) > 64 * 1024)
    return set_error(ctx, MTG_ERR_TOO_LARGE, "per-trajectory coefficients exceed LDS (reduce K)");
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int V = K + 1, h = N / 2;
  const size_t nB = (size_t)batch, b_grad = sizeof(double) * nB * D * V * h;
  const double *d_vals, *d_times;
  const uint8_t* d_mask;
  const float* d_grid;
  double *d_cost, *d_grad;
  uint8_t* d_coll;
  int32_t *d_nev, *d_stat;
  Staged st(ctx, flags);
  st.in(&d_vals, vertex_values, sizeof(double) * nB * V * h * D);
  st.in(&d_mask, fixed_mask, grad_out ? nB * V : 0);
  st.in(&d_times, times, sizeof(double) * nB * K);
  st.in(&d_grid, grid->distance, grid_bytes(*grid));
  st.out(&d_cost, cost_out, sizeof(double) * nB);
  st.out(&d_grad, grad_out, b_grad);
  st.out(&d_coll, collision_out, nB);
  st.out(&d_nev, n_evaluated_out, sizeof(int32_t) * nB);
  st.out(&d_stat, status, sizeof(int32_t) * nB);
  if (int rc = st.upload()) return rc;
  if (d_grad) MTG_HIP_TRY(ctx, hipMemsetAsync(d_grad, 0, b_grad, ctx->stream));
  MTG_HIP_TRY(ctx, time_begin(ctx));
  MTG_HIP_TRY(ctx, mtg::launch_collision_cost(N, d_vals, d_mask, d_times, *grid, d_grid, *params, d_cost, d_grad, d_coll,
                                              d_nev, d_stat, batch, K, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  return st.finish();
}

int mtg_collision_cost_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                    const double* vertex_values, const uint8_t* fixed_mask, const double* times,
                                    const mtg_sdf_grid* grid, const mtg_collision_params* params, double* cost_out,
                                    double* grad_out, uint8_t* collision_out, int32_t* n_evaluated_out, int32_t* status,
                                    unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_collision(ctx, N, D, 1, batch, grid, params)) return rc;
  if (batch == 0) return MTG_OK;
  try {
    int k_max = 0;
    std::vector<int64_t> so;
    if (int rc = ragged_check_counts(ctx, batch, seg_count, &k_max, &so)) return rc;
    if (!vertex_values || !times || !cost_out || !grid->distance || (grad_out && !fixed_mask))
      return set_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                       "vertex_values, times, cost_out and grid->distance are required; grad_out needs fixed_mask");
    if (mtg::collision_lds_bytes(N, k_max) > 64 * 1024)
      return set_error(ctx, MTG_ERR_TOO_LARGE, "the longest trajectory's coefficients exceed LDS (reduce its K)");
    std::lock_guard<std::mutex> g(ctx->mu);
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // one launch on the caller's CSR arrays: nothing is copied on the device
    const int h = N / 2;
    const size_t nB = (size_t)batch, totS = (size_t)so.back(), totV = totS + nB;
    const size_t b_grad = sizeof(double) * totV * D * h;
    const double *d_vals, *d_times;
    const uint8_t* d_mask;
    const float* d_grid;
    double *d_cost, *d_grad;
    uint8_t* d_coll;
    int32_t *d_nev, *d_stat;
    Staged st(ctx, flags);
    st.in(&d_vals, vertex_values, sizeof(double) * totV * h * D);
    st.in(&d_mask, fixed_mask, grad_out ? totV : 0);
    st.in(&d_times, times, sizeof(double) * totS);
    st.in(&d_grid, grid->distance, grid_bytes(*grid));
    st.out(&d_cost, cost_out, sizeof(double) * nB);
    st.out(&d_grad, grad_out, b_grad);
    st.out(&d_coll, collision_out, nB);
    st.out(&d_nev, n_evaluated_out, sizeof(int32_t) * nB);
    st.out(&d_stat, status, sizeof(int32_t) * nB);
    if (int rc = ragged_wait_last(ctx)) return rc;
    if (int rc = st.upload()) return rc;
    const size_t b_so = sizeof(int64_t) * so.size();
    MTG_HIP_TRY(ctx, ensure(&ctx->ragged, &ctx->ragged_bytes, align_up(b_so)));
    if (int rc = ragged_upload(ctx, b_so, ctx->ragged, [&](void* p) { std::memcpy(p, so.data(), b_so); })) return rc;
    if (d_grad) MTG_HIP_TRY(ctx, hipMemsetAsync(d_grad, 0, b_grad, ctx->stream));
    MTG_HIP_TRY(ctx, time_begin(ctx));
    MTG_HIP_TRY(ctx, mtg::launch_collision_cost_ragged(N, k_max, batch, static_cast<const int64_t*>(ctx->ragged), d_vals,
                                                       d_mask, d_times, *grid, d_grid, *params, d_cost, d_grad, d_coll,
                                                       d_nev, d_stat, ctx->stream));
    MTG_HIP_TRY(ctx, time_end(ctx));
    if (int rc = ragged_mark_last(ctx)) return rc;
    return st.finish();
  } catch (const std::bad_alloc&) {
    return set_error(ctx, MTG_ERR_OUT_OF_MEMORY, "ragged collision cost: out of host memory");
  }
}

int mtg_collision_time_gradient_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* vertex_values,
                                      const double* times, const mtg_sdf_grid* grid, const mtg_collision_params* params,
                                      double increment_time, double* grad_t_out, double* side_cost_out,
                                      int32_t* side_evaluated_out, int32_t* segments_walked_out, int32_t* status,
                                      unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_collision(ctx, N, D, K, batch, grid, params)) return rc;
  if (!(increment_time > 0.0 && increment_time <= DBL_MAX))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "increment_time must be > 0 and finite");
  if (batch == 0) return MTG_OK;
  if (!vertex_values || !times || !grad_t_out || !grid->distance)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "vertex_values, times, grad_t_out and grid->distance are required");
  if (mtg::collision_time_lds_bytes(N, K) > 64 * 1024 || batch > 0x7fffffff)
    return set_error(ctx, MTG_ERR_TOO_LARGE, "one trajectory's coefficients and walk records exceed LDS (reduce K)");
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int V = K + 1, h = N / 2;
  const size_t nB = (size_t)batch;
  const double *d_vals, *d_times;
  const float* d_grid;
  double *d_grad, *d_sc;
  int32_t *d_se, *d_wk, *d_stat;
  Staged st(ctx, flags);
  st.in(&d_vals, vertex_values, sizeof(double) * nB * V * h * D);
  st.in(&d_times, times, sizeof(double) * nB * K);
  st.in(&d_grid, grid->distance, grid_bytes(*grid));
  st.out(&d_grad, grad_t_out, sizeof(double) * nB * K);
  st.out(&d_sc, side_cost_out, sizeof(double) * nB * K * 2);
  st.out(&d_se, side_evaluated_out, sizeof(int32_t) * nB * K * 2);
  st.out(&d_wk, segments_walked_out, sizeof(int32_t) * nB);
  st.out(&d_stat, status, sizeof(int32_t) * nB);
  if (int rc = st.upload()) return rc;
  MTG_HIP_TRY(ctx, time_begin(ctx));
  MTG_HIP_TRY(ctx, mtg::launch_collision_time_gradient(N, d_vals, d_times, *grid, d_grid, *params, increment_time, d_grad,
                                                       d_sc, d_se, d_wk, d_stat, batch, K, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  return st.finish();
}

int mtg_soft_constraint_cost_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* vertex_values,
                                   const uint8_t* fixed_mask, const double* times,
                                   const mtg_soft_constraint_params* params, double* cost_out, double* grad_out,
                                   mtg_extremum* maxima_out, int32_t* status, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (N < 6 || N > 12 || (N % 2)) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "N must be 6, 8, 10 or 12");
  if (D < 1 || D > 4) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "the soft-constraint term needs 1 <= D <= 4");
  if (K < 1 || batch < 0) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need K >= 1, batch >= 0");
  if (int rc = check_soft_params(ctx, N, params, "params with 1 <= n_constraints <= 8 are required")) return rc;
  const int C = params->n_constraints;
  if (batch == 0) return MTG_OK;
  if (!vertex_values || !times || !cost_out || (grad_out && !fixed_mask))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                     "vertex_values, times and cost_out are required; grad_out needs fixed_mask");
  if (mtg::soft_constraint_threads(N, D, K, C) == 0 || batch > 0x7fffffff)
    return set_error(ctx, MTG_ERR_TOO_LARGE, "per-trajectory working set exceeds LDS (reduce K), or batch >= 2^31");
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int V = K + 1, h = N / 2;
  const size_t nB = (size_t)batch;
  const double *d_vals, *d_times;
  const uint8_t* d_mask;
  double *d_cost, *d_grad;
  mtg_extremum* d_max;
  int32_t* d_stat;
  Staged st(ctx, flags);
  st.in(&d_vals, vertex_values, sizeof(double) * nB * V * h * D);
  st.in(&d_mask, fixed_mask, grad_out ? nB * V : 0);
  st.in(&d_times, times, sizeof(double) * nB * K);
  st.out(&d_cost, cost_out, sizeof(double) * nB);
  st.out(&d_grad, grad_out, sizeof(double) * nB * D * V * h);
  st.out(&d_max, maxima_out, sizeof(mtg_extremum) * nB * C);
  st.out(&d_stat, status, sizeof(int32_t) * nB);
  if (int rc = st.upload()) return rc;
  MTG_HIP_TRY(ctx, time_begin(ctx));  // (the kernel writes every entry of grad_out itself)
  MTG_HIP_TRY(ctx, mtg::launch_soft_constraint_cost(N, d_vals, d_mask, d_times, *params, d_cost, d_grad, d_max, d_stat,
                                                    batch, K, D, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  return st.finish();
}

int mtg_time_jacobian_batch(mtg_ctx* ctx, int N, int D, int K, int derivative_to_optimize,
                            int64_t batch, const double* vertex_values, const double* times,
                            int n_candidates, const double* scales, double increment_time,
                            double* cost_out, double* jac_out, unsigned flags) {
  int rc = check_shape(ctx, N, D, K, derivative_to_optimize, batch);
  if (rc != MTG_OK) return rc;
  if (n_candidates < 1) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "n_candidates must be >= 1");
  if (!(increment_time >= 0.0) || increment_time > DBL_MAX)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "increment_time must be finite and >= 0");
  if (batch == 0) return MTG_OK;
  if (!vertex_values || !times || !scales || !cost_out)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "vertex_values, times, scales, cost_out are required");
  if (mtg::time_jacobian_lds_bytes(N, D, K, n_candidates) > 160 * 1024)
    return set_error(ctx, MTG_ERR_TOO_LARGE, "per-block cost tables exceed LDS (reduce K or D)");
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int V = K + 1, h = N / 2, C = n_candidates;
  const size_t nB = (size_t)batch;
  const double *d_vals, *d_times, *d_scales;
  double *d_cost, *d_jac;
  Staged st(ctx, flags);
  st.in(&d_vals, vertex_values, sizeof(double) * nB * V * h * D);
  st.in(&d_times, times, sizeof(double) * nB * K);
  st.in(&d_scales, scales, sizeof(double) * (size_t)C * K);
  st.out(&d_cost, cost_out, sizeof(double) * nB * C);
  st.out(&d_jac, jac_out, sizeof(double) * nB * C * K);
  if (int rc = st.upload()) return rc;
  MTG_HIP_TRY(ctx, time_begin(ctx));
  MTG_HIP_TRY(ctx, mtg::launch_time_jacobian(N, derivative_to_optimize, d_vals, d_times, d_scales, d_cost, d_jac,
                                             increment_time, batch, K, D, C, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  return st.finish();
}

// The objective in the optimiser's variables.  Launch sequence on the context's stream, no host
// synchronisation in between: unpack | cost | [collision] | [soft] | [jacobian |
// collision-time] | combine.  The component LAUNCHERS are called, not the entry points above, so
// nothing is staged twice; intermediates live in ctx->workspace.
int mtg_objective_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* values,
                        const uint8_t* fixed_mask, const double* times, const double* x, int64_t x_stride,
                        const mtg_objective_params* params, const mtg_sdf_grid* grid,
                        const mtg_collision_params* collision, const mtg_soft_constraint_params* soft,
                        double* cost_out, double* grad_out, double* weighted_costs_out, uint8_t* collision_out,
                        mtg_objective_state* state, const mtg_objective_parts* parts, int32_t* status, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!params) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "params are required");
  const int obj = params->objective;
  if (obj < MTG_OBJECTIVE_FREE_CONSTRAINTS || obj > MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION_AND_TIME)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "objective not covered (the solve-based objectives are not)");
  if (params->reserved != 0)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "reserved must be 0 (the numerical-gradient switches are not covered)");
  const bool with_coll = obj != MTG_OBJECTIVE_FREE_CONSTRAINTS;
  const bool with_time = obj == MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION_AND_TIME;
  const bool with_soft = params->use_soft_constraints != 0;
  const bool with_grad = grad_out != nullptr;
  const int r = params->derivative_to_optimize;
  int rc = check_shape(ctx, N, D, K, r, batch);
  if (rc != MTG_OK) return rc;
  if (with_coll) {
    rc = check_collision(ctx, N, D, K, batch, grid, collision, "grid and collision params are required");
    if (rc != MTG_OK) return rc;
    if (with_time && !(params->increment_time > 0.0 && params->increment_time <= DBL_MAX))
      return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "increment_time must be > 0 and finite");
  } else if (D > 4) {
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "objective 0 needs 1 <= D <= 4");
  }
  if (with_soft != (soft != nullptr))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "soft params are required iff use_soft_constraints");
  int C = 0;
  if (with_soft) {
    if (N < 6 || D > 4) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "the soft-constraint term needs N >= 6, D <= 4");
    rc = check_soft_params(ctx, N, soft, "need 1 <= n_constraints <= 8");
    if (rc != MTG_OK) return rc;
    C = soft->n_constraints;
  }
  if (x_stride < 0) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "x_stride must be >= 0");
  if (batch == 0) return MTG_OK;
  if (!values || !fixed_mask || !cost_out || !x || (!with_time && !times) ||
      (with_coll && !grid->distance))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                     "values, fixed_mask, x, cost_out (objectives 0, 1: times; 1, 2: grid->distance) are required");
  const int V = K + 1, h = N / 2;
  const bool dev = flags & MTG_FLAG_DEVICE_PTRS;
  const int nt = with_time ? K : 0;
  if (!dev) {  // the longest row must fit (a device-pointer call checks per trajectory in the unpack kernel)
    int64_t longest = 0;
    for (int64_t b = 0; b < batch; ++b)
      longest = std::max<int64_t>(longest, nt + (int64_t)D * mtg::objective_n_free(fixed_mask + b * V, V, h));
    if (x_stride < longest) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "x_stride is shorter than the longest row");
  }
  if (mtg::cost_lds_bytes(N, D, K) > 64 * 1024 || (with_coll && mtg::collision_lds_bytes(N, K) > 64 * 1024) ||
      (with_soft && mtg::soft_constraint_threads(N, D, K, C) == 0) ||
      (with_time && with_grad &&
       (mtg::collision_time_lds_bytes(N, K) > 64 * 1024 || mtg::time_jacobian_lds_bytes(N, D, K, 1) > 160 * 1024)) ||
      batch > 0x7fffffff || (double)batch * (double)std::max<int64_t>((int64_t)V * h * D, x_stride) > 5e11)
    return set_error(ctx, MTG_ERR_TOO_LARGE, "a component's per-trajectory working set exceeds LDS (reduce K), or the batch is too large");
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));

  // ---- workspace: every intermediate of the call
  const size_t nB = (size_t)batch;
  const size_t b_vv = sizeof(double) * nB * V * h * D, b_T = sizeof(double) * nB * K, b_s = sizeof(double) * nB,
               b_g = with_grad ? sizeof(double) * nB * D * V * h : 0, b_jt = with_time && with_grad ? b_T : 0,
               b_i = sizeof(int32_t) * nB;
  size_t woff = 0;
  auto take = [&](size_t bytes) {
    const size_t o = woff;
    woff = align_up(woff + bytes);
    return o;
  };
  const size_t w_vv = take(b_vv), w_T = take(b_T), w_ones = take(sizeof(double) * K), w_Jd = take(b_s), w_Jc = take(b_s),
               w_Jsc = take(b_s), w_Jt = take(b_s), w_Jd2 = take(b_s), w_gd = take(b_g), w_gc = take(with_coll ? b_g : 0),
               w_gsc = take(with_coll && with_soft ? b_g : 0), w_jd = take(b_jt), w_jc = take(b_jt), w_coll = take(nB),
               w_nf = take(b_i), w_su = take(b_i), w_sc = take(b_i), w_ss = take(b_i), w_st = take(b_i);
  MTG_HIP_TRY(ctx, ensure(&ctx->workspace, &ctx->workspace_bytes, std::max<size_t>(woff, 256)));
  char* ws = static_cast<char*>(ctx->workspace);
  auto wd = [&](size_t o) { return reinterpret_cast<double*>(ws + o); };
  auto wi = [&](size_t o) { return reinterpret_cast<int32_t*>(ws + o); };

  // ---- staging of a host-pointer call: inputs and the objective's own outputs (the parts are copied
  // out of the workspace)
  const size_t b_x = sizeof(double) * nB * (size_t)x_stride;
  const double *d_x, *d_vals, *d_times;
  const uint8_t* d_mask;
  const float* d_grid;
  double *d_cost, *d_grad, *d_w;
  uint8_t* d_co;
  mtg_objective_state* d_state;
  int32_t* d_stat;
  Staged st(ctx, flags);
  st.in(&d_x, x, b_x);
  st.in(&d_vals, values, b_vv);
  st.in(&d_mask, fixed_mask, nB * V);
  st.in(&d_times, times, with_time ? 0 : b_T);
  st.in(&d_grid, with_coll ? grid->distance : nullptr, with_coll ? grid_bytes(*grid) : 0);
  st.out(&d_cost, cost_out, b_s);
  st.out(&d_grad, grad_out, b_x);
  st.out(&d_w, weighted_costs_out, 4 * b_s);
  st.out(&d_co, collision_out, nB);
  st.inout(&d_state, state, sizeof(mtg_objective_state) * nB);
  st.out(&d_stat, status, b_i);
  rc = st.upload();
  if (rc != MTG_OK) return rc;

  // ---- the launches
  MTG_HIP_TRY(ctx, time_begin(ctx, false));
  mtg::ObjectiveUnpackArgs ua{d_x, d_vals, d_mask, with_time ? nullptr : d_times, wd(w_vv), wd(w_T), wi(w_nf), wi(w_su),
                              wd(w_ones), batch, x_stride, K, V, h, D};
  MTG_HIP_TRY(ctx, mtg::launch_objective_unpack(ua, ctx->stream));
  // (entries >= n_free of grad_d / grad_c are read by nobody but a caller of the parts)
  if (with_grad && parts && parts->grad_d) MTG_HIP_TRY(ctx, hipMemsetAsync(wd(w_gd), 0, b_g, ctx->stream));
  if (with_grad && with_coll && parts && parts->grad_c) MTG_HIP_TRY(ctx, hipMemsetAsync(wd(w_gc), 0, b_g, ctx->stream));
  MTG_HIP_TRY(ctx, mtg::launch_cost_at_times(N, r, wd(w_vv), d_mask, wd(w_T), wd(w_ones), wd(w_Jd),
                                             with_grad ? wd(w_gd) : nullptr, batch, K, D, 1, ctx->stream));
  if (with_coll)
    MTG_HIP_TRY(ctx, mtg::launch_collision_cost(N, wd(w_vv), d_mask, wd(w_T), *grid, d_grid, *collision, wd(w_Jc),
                                                with_grad ? wd(w_gc) : nullptr, reinterpret_cast<uint8_t*>(ws + w_coll),
                                                nullptr, wi(w_sc), batch, K, ctx->stream));
  const bool soft_grad = with_grad && with_coll;  // objective 0 uses the soft-constraint cost only
  if (with_soft)
    MTG_HIP_TRY(ctx, mtg::launch_soft_constraint_cost(N, wd(w_vv), d_mask, wd(w_T), *soft, wd(w_Jsc),
                                                      soft_grad ? wd(w_gsc) : nullptr, nullptr, wi(w_ss), batch, K, D,
                                                      ctx->stream));
  if (with_time && with_grad) {
    MTG_HIP_TRY(ctx, mtg::launch_time_jacobian(N, r, wd(w_vv), wd(w_T), wd(w_ones), wd(w_Jd2), wd(w_jd),
                                               params->increment_time, batch, K, D, 1, ctx->stream));
    MTG_HIP_TRY(ctx, mtg::launch_collision_time_gradient(N, wd(w_vv), wd(w_T), *grid, d_grid, *collision,
                                                         params->increment_time, wd(w_jc), nullptr, nullptr, nullptr,
                                                         wi(w_st), batch, K, ctx->stream));
  }
  mtg::ObjectiveCombineArgs ca{};
  ca.J_d = wd(w_Jd);
  ca.J_c = with_coll ? wd(w_Jc) : nullptr;
  ca.J_sc = with_soft ? wd(w_Jsc) : nullptr;
  ca.grad_d = with_grad ? wd(w_gd) : nullptr;
  ca.grad_c = with_grad && with_coll ? wd(w_gc) : nullptr;
  ca.grad_sc = soft_grad && with_soft ? wd(w_gsc) : nullptr;
  ca.dJd_dt = with_time && with_grad ? wd(w_jd) : nullptr;
  ca.dJc_dt = with_time && with_grad ? wd(w_jc) : nullptr;
  ca.times = wd(w_T);
  ca.collision = with_coll ? reinterpret_cast<const uint8_t*>(ws + w_coll) : nullptr;
  ca.n_free = wi(w_nf);
  ca.st_unpack = wi(w_su);
  ca.st_collision = with_coll ? wi(w_sc) : nullptr;
  ca.st_soft = with_soft ? wi(w_ss) : nullptr;
  ca.st_collision_time = with_time && with_grad ? wi(w_st) : nullptr;
  ca.cost_out = d_cost;
  ca.grad_out = d_grad;
  ca.weighted = d_w;
  ca.J_t_out = wd(w_Jt);
  ca.collision_out = d_co;
  ca.state = d_state;
  ca.status = d_stat;
  ca.B = batch;
  ca.x_stride = x_stride;
  ca.K = K, ca.V = V, ca.h = h, ca.D = D;
  ca.rule = mtg::ObjectiveRule{obj, params->w_d, params->w_c, params->w_t, params->w_sc, params->is_collision_safe,
                               params->is_coll_raise_first_iter, params->add_coll_raise};
  MTG_HIP_TRY(ctx, mtg::launch_objective_combine(ca, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));

  // ---- the parts (from the workspace) and, for host pointers, the outputs
  const hipMemcpyKind out_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (parts) {
    const struct { double* dst; size_t off, bytes; bool have; } pc[] = {
        {parts->J_d, w_Jd, b_s, true}, {parts->J_c, w_Jc, b_s, with_coll}, {parts->J_sc, w_Jsc, b_s, with_soft},
        {parts->J_t, w_Jt, b_s, true}, {parts->dJd_dt, w_jd, b_jt, b_jt != 0}, {parts->dJc_dt, w_jc, b_jt, b_jt != 0},
        {parts->grad_d, w_gd, b_g, with_grad}, {parts->grad_c, w_gc, b_g, with_grad && with_coll},
        {parts->grad_sc, w_gsc, b_g, soft_grad && with_soft}};
    for (const auto& q : pc)
      if (q.dst && q.have && q.bytes)
        MTG_HIP_TRY(ctx, hipMemcpyAsync(q.dst, ws + q.off, q.bytes, out_kind, ctx->stream));
  }
  return st.finish();
}

// The two gradient-free objectives in the segment times.  Launch sequence on the context's stream, no
// host synchronisation in between:
//   objective 3: times-unpack | solve (flags 0) | assemble | [soft] | [collision at coeff_times] | combine
//   objective 4: unpack | cost | [soft] | [vertex map] | combine
// As in mtg_objective_batch the component LAUNCHERS are called and intermediates live in ctx->workspace.
int mtg_objective_time_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* values,
                             const uint8_t* fixed_mask, const double* x, int64_t x_stride,
                             const mtg_objective_time_params* params, const double* coeff_times,
                             const mtg_sdf_grid* grid, const mtg_collision_params* collision,
                             const mtg_soft_constraint_params* constraints, double* cost_out,
                             double* weighted_costs_out, uint8_t* collision_out, double* constraint_values_out,
                             mtg_extremum* maxima_out, double* free_out, double* coeffs_out,
                             mtg_objective_state* state, const mtg_objective_parts* parts, int32_t* status,
                             unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!params) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "params are required");
  const int obj = params->objective;
  if (obj != MTG_OBJECTIVE_TIME && obj != MTG_OBJECTIVE_TIME_AND_CONSTRAINTS)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "objective must be MTG_OBJECTIVE_TIME or MTG_OBJECTIVE_TIME_AND_CONSTRAINTS");
  if (params->reserved != 0) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "reserved must be 0");
  const bool solve = obj == MTG_OBJECTIVE_TIME;
  const bool with_coll = solve && params->w_c > 0.0;
  const bool with_soft = params->use_soft_constraints != 0;
  const bool with_max = with_soft || constraint_values_out || maxima_out;  // the maxima search runs
  const int r = params->derivative_to_optimize;
  int rc = check_shape(ctx, N, D, K, r, batch);
  if (rc != MTG_OK) return rc;
  if (with_coll) {
    rc = check_collision(ctx, N, D, K, batch, grid, collision, "w_c > 0 needs grid and collision params");
    if (rc != MTG_OK) return rc;
    if (!coeff_times) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "w_c > 0 needs coeff_times");
  } else if (D > 4 || grid || collision || coeff_times) {
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                     "without a collision term (objective 4, or w_c <= 0) 1 <= D <= 4 and grid, collision, coeff_times are NULL");
  }
  int C = 0;
  if (with_max) {
    if (N < 6) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "the soft-constraint search needs N >= 6");
    rc = check_soft_params(ctx, N, constraints, "constraints with 1 <= n_constraints <= 8 are required");
    if (rc != MTG_OK) return rc;
    C = constraints->n_constraints;
  }
  if (parts && (parts->dJd_dt || parts->dJc_dt || parts->grad_d || parts->grad_c || parts->grad_sc))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "the gradient fields of parts must be NULL (these objectives have no gradient)");
  if (x_stride < 0) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "x_stride must be >= 0");
  if (batch == 0) return MTG_OK;
  if (!values || !fixed_mask || !cost_out || !x || (with_coll && !grid->distance))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "values, fixed_mask, x, cost_out (w_c > 0: grid->distance) are required");
  const int V = K + 1, h = N / 2;
  const bool dev = flags & MTG_FLAG_DEVICE_PTRS;
  if (!dev) {  // the longest row must fit (a device-pointer call checks per trajectory in the unpack kernels)
    int64_t longest = K;
    for (int64_t b = 0; !solve && b < batch; ++b)
      longest = std::max<int64_t>(longest, K + (int64_t)D * mtg::objective_n_free(fixed_mask + b * V, V, h));
    if (x_stride < longest) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "x_stride is shorter than the longest row");
  }
  const bool with_map = !solve && coeffs_out;
  if ((!solve && mtg::cost_lds_bytes(N, D, K) > 64 * 1024) || (with_coll && mtg::collision_lds_bytes(N, K) > 64 * 1024) ||
      (with_max && mtg::soft_constraint_threads(N, D, K, C) == 0) || (with_map && !mtg::vertex_map_fits(N, D, K)) ||
      batch > 0x7fffffff ||
      (double)batch * (double)std::max<int64_t>(std::max<int64_t>((int64_t)V * h * D, (int64_t)K * D * N), x_stride) > 5e11)
    return set_error(ctx, MTG_ERR_TOO_LARGE, "a component's per-trajectory working set exceeds LDS (reduce K), or the batch is too large");
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));

  // ---- workspace: every intermediate of the call (an output the caller asked for is written in place)
  const size_t nB = (size_t)batch;
  const size_t b_vv = sizeof(double) * nB * V * h * D, b_T = sizeof(double) * nB * K, b_s = sizeof(double) * nB,
               b_free = sizeof(double) * nB * D * V * h, b_co = sizeof(double) * nB * K * D * N, b_i = sizeof(int32_t) * nB,
               b_mx = sizeof(mtg_extremum) * nB * C;
  const bool dlx = solve && mtg::solve_kernel(N, D, K, 0, r, batch) == MTG_KERNEL_DLX;
  size_t woff = 0;
  auto take = [&](size_t bytes) {
    const size_t o = woff;
    woff = align_up(woff + bytes);
    return o;
  };
  const size_t w_vv = take(b_vv), w_T = take(b_T), w_ones = take(solve ? 0 : sizeof(double) * K), w_ct = take(b_s),
               w_Jc = take(b_s), w_Jsc = take(b_s), w_Jt = take(b_s), w_free = take(solve && !free_out ? b_free : 0),
               w_co = take(solve && !coeffs_out ? b_co : 0), w_mx = take(with_max && !maxima_out ? b_mx : 0),
               w_coll = take(nB), w_nf = take(b_i), w_su = take(b_i), w_sv = take(b_i), w_sc = take(b_i), w_ss = take(b_i),
               w_dlx = take(dlx ? mtg::dlx_workspace_bytes(N, D, K, batch) : 0);
  MTG_HIP_TRY(ctx, ensure(&ctx->workspace, &ctx->workspace_bytes, std::max<size_t>(woff, 256)));
  char* ws = static_cast<char*>(ctx->workspace);
  auto wd = [&](size_t o) { return reinterpret_cast<double*>(ws + o); };
  auto wi = [&](size_t o) { return reinterpret_cast<int32_t*>(ws + o); };

  // ---- staging of a host-pointer call (the parts are copied out of the workspace)
  const double *d_x, *d_vals, *d_ctimes;
  const uint8_t* d_mask;
  const float* d_grid;
  double *d_cost, *d_w, *d_cv, *d_free, *d_co;
  mtg_extremum* d_max;
  uint8_t* d_coll;
  mtg_objective_state* d_state;
  int32_t* d_stat;
  Staged st(ctx, flags);
  st.in(&d_x, x, sizeof(double) * nB * (size_t)x_stride);
  st.in(&d_vals, values, b_vv);
  st.in(&d_mask, fixed_mask, nB * V);
  st.in(&d_ctimes, coeff_times, with_coll ? b_T : 0);
  st.in(&d_grid, with_coll ? grid->distance : nullptr, with_coll ? grid_bytes(*grid) : 0);
  st.out(&d_cost, cost_out, b_s);
  st.out(&d_w, weighted_costs_out, 4 * b_s);
  st.out(&d_coll, collision_out, nB);
  st.out(&d_cv, constraint_values_out, sizeof(double) * nB * C);
  st.out(&d_max, maxima_out, b_mx);
  st.out(&d_free, free_out, b_free);
  st.out(&d_co, coeffs_out, b_co);
  st.inout(&d_state, state, sizeof(mtg_objective_state) * nB);
  st.out(&d_stat, status, b_i);
  rc = st.upload();
  if (rc != MTG_OK) return rc;

  // ---- the launches
  double* p_free = d_free ? d_free : (solve ? wd(w_free) : nullptr);
  double* p_co = d_co ? d_co : (solve ? wd(w_co) : nullptr);
  mtg_extremum* p_max = d_max ? d_max : (with_max ? reinterpret_cast<mtg_extremum*>(ws + w_mx) : nullptr);
  uint8_t* p_coll = reinterpret_cast<uint8_t*>(ws + w_coll);
  MTG_HIP_TRY(ctx, time_begin(ctx, false));
  if (solve) {
    mtg::ObjectiveTimesUnpackArgs ta{d_x, wd(w_T), wi(w_su), batch, x_stride, K};
    MTG_HIP_TRY(ctx, mtg::launch_objective_times_unpack(ta, ctx->stream));
    MTG_HIP_TRY(ctx, hipMemsetAsync(p_free, 0, b_free, ctx->stream));  // entries beyond n_free stay zero
    mtg::SolveArgs sa{};
    sa.values = d_vals;
    sa.mask = d_mask;
    sa.times = wd(w_T);
    sa.coeffs = p_co;
    sa.free_out = p_free;
    sa.n_free_out = wi(w_nf);
    sa.cost_out = wd(w_ct);
    sa.status = wi(w_sv);
    sa.B = batch;
    sa.K = K;
    sa.D = D;
    sa.r = r;
    sa.n_cand = 1;
    if (dlx) {
      sa.work = wd(w_dlx);
      sa.work_bytes = (int64_t)mtg::dlx_workspace_bytes(N, D, K, batch);
    }
    MTG_HIP_TRY(ctx, mtg::launch_solve(N, sa, ctx->stream, 0));
    mtg::ObjectiveAssembleArgs aa{d_vals, d_mask, p_free, wd(w_vv), batch, V, h, D};
    MTG_HIP_TRY(ctx, mtg::launch_objective_assemble(aa, ctx->stream));
  } else {
    mtg::ObjectiveUnpackArgs ua{d_x, d_vals, d_mask, nullptr, wd(w_vv), wd(w_T), wi(w_nf), wi(w_su), wd(w_ones),
                                batch, x_stride, K, V, h, D};
    MTG_HIP_TRY(ctx, mtg::launch_objective_unpack(ua, ctx->stream));
    MTG_HIP_TRY(ctx, mtg::launch_cost_at_times(N, r, wd(w_vv), d_mask, wd(w_T), wd(w_ones), wd(w_ct), nullptr, batch, K, D,
                                               1, ctx->stream));
  }
  if (with_max)
    MTG_HIP_TRY(ctx, mtg::launch_soft_constraint_cost(N, wd(w_vv), d_mask, wd(w_T), *constraints, wd(w_Jsc), nullptr, p_max,
                                                      wi(w_ss), batch, K, D, ctx->stream));
  if (with_coll)
    MTG_HIP_TRY(ctx, mtg::launch_collision_cost(N, wd(w_vv), d_mask, wd(w_T), *grid, d_grid, *collision, wd(w_Jc), nullptr,
                                                p_coll, nullptr, wi(w_sc), batch, K, ctx->stream, d_ctimes));
  if (with_map) MTG_HIP_TRY(ctx, mtg::launch_vertex_map(true, N, wd(w_vv), wd(w_T), d_co, batch, K, D, ctx->stream));
  mtg::ObjectiveTimeCombineArgs ca{};
  ca.cost_traj = wd(w_ct);
  ca.J_c = with_coll ? wd(w_Jc) : nullptr;
  ca.J_sc = with_soft ? wd(w_Jsc) : nullptr;
  ca.times = wd(w_T);
  ca.collision = with_coll ? p_coll : nullptr;
  ca.st_unpack = wi(w_su);
  ca.st_solve = solve ? wi(w_sv) : nullptr;
  ca.st_soft = with_max ? wi(w_ss) : nullptr;
  ca.st_collision = with_coll ? wi(w_sc) : nullptr;
  ca.maxima = p_max;
  ca.x = d_x;
  ca.n_free = wi(w_nf);
  for (int c = 0; c < C; ++c) ca.limit[c] = constraints->limit[c];
  ca.C = C;
  ca.cost_out = d_cost;
  ca.weighted = d_w;
  ca.J_t_out = wd(w_Jt);
  ca.constraint_values = d_cv;
  ca.free_out = d_free;
  ca.coeffs_out = d_co;
  ca.maxima_out = d_max;
  ca.collision_out = d_coll;
  ca.state = d_state;
  ca.status = d_stat;
  ca.B = batch;
  ca.x_stride = x_stride;
  ca.K = K, ca.V = V, ca.h = h, ca.D = D, ca.N = N;
  ca.rule = mtg::ObjectiveTimeRule{obj, params->time_penalty, params->w_c};
  MTG_HIP_TRY(ctx, mtg::launch_objective_time_combine(ca, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));

  // ---- the parts (from the workspace) and, for host pointers, the outputs
  if (parts) {
    const hipMemcpyKind out_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const struct { double* dst; size_t off; bool have; } pc[] = {{parts->J_d, w_ct, !solve}, {parts->J_c, w_Jc, with_coll},
                                                                  {parts->J_sc, w_Jsc, with_max}, {parts->J_t, w_Jt, true}};
    for (const auto& q : pc)
      if (q.dst && q.have) MTG_HIP_TRY(ctx, hipMemcpyAsync(q.dst, ws + q.off, b_s, out_kind, ctx->stream));
  }
  return st.finish();
}

namespace {

// Shared body of the two vertex <-> coefficient maps: [B][V][h][D] <-> [B][K][D][N].
int run_vertex_map(mtg_ctx* ctx, bool to_coeffs, int N, int D, int K, int64_t batch, const double* in,
                   const double* times, double* out, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_order(ctx, N)) return rc;
  if (int rc = check_dims(ctx, D, K, batch)) return rc;
  if (!mtg::vertex_map_fits(N, D, K))
    return set_error(ctx, MTG_ERR_TOO_LARGE, "per-trajectory arrays exceed the LDS staging (reduce K or D)");
  if (batch == 0) return MTG_OK;
  if (!in || !times || !out) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "input, times and output are required");
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int V = K + 1, h = N / 2;
  const size_t nB = (size_t)batch, b_vals = sizeof(double) * nB * V * h * D, b_coef = sizeof(double) * nB * K * D * N;
  const double *d_in, *d_times;
  double* d_out;
  Staged st(ctx, flags);
  st.in(&d_in, in, to_coeffs ? b_vals : b_coef);
  st.in(&d_times, times, sizeof(double) * nB * K);
  st.out(&d_out, out, to_coeffs ? b_coef : b_vals);
  if (int rc = st.upload()) return rc;
  MTG_HIP_TRY(ctx, time_begin(ctx));
  MTG_HIP_TRY(ctx, mtg::launch_vertex_map(to_coeffs, N, d_in, d_times, d_out, batch, K, D, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  return st.finish();
}

}  // namespace

int mtg_coefficients_from_vertices_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch,
                                         const double* vertex_values, const double* times, double* coeffs,
                                         unsigned flags) {
  return run_vertex_map(ctx, true, N, D, K, batch, vertex_values, times, coeffs, flags);
}

int mtg_vertex_derivatives_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* coeffs,
                                 const double* times, double* vertex_values, unsigned flags) {
  return run_vertex_map(ctx, false, N, D, K, batch, coeffs, times, vertex_values, flags);
}

namespace {

// Shared body of the two maps on a CSR batch: [sum K + B][h][D] <-> [sum K][D][N].
// The segment offsets go to ctx->ragged, then one launch over tiles of packed segments.
int run_vertex_map_ragged(mtg_ctx* ctx, bool to_coeffs, int N, int D, int64_t batch, const int32_t* seg_count,
                          const double* in, const double* times, double* out, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_order(ctx, N)) return rc;
  if (D < 1 || batch < 0) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need D >= 1, batch >= 0");
  if (mtg::vertex_ragged_tile(N, D) < 1)
    return set_error(ctx, MTG_ERR_TOO_LARGE, "one segment's arrays exceed the LDS staging (reduce D)");
  if (batch == 0) return MTG_OK;
  try {
    int k_max = 0;
    std::vector<int64_t> so;
    if (int rc = ragged_check_counts(ctx, batch, seg_count, &k_max, &so)) return rc;
    if (!in || !times || !out) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "input, times and output are required");
    std::lock_guard<std::mutex> g(ctx->mu);
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int h = N / 2;
    const size_t nB = (size_t)batch, totS = (size_t)so.back();
    const size_t b_vals = sizeof(double) * (totS + nB) * h * D, b_coef = sizeof(double) * totS * D * N;
    const double *d_in, *d_times;
    double* d_out;
    Staged st(ctx, flags);
    st.in(&d_in, in, to_coeffs ? b_vals : b_coef);
    st.in(&d_times, times, sizeof(double) * totS);
    st.out(&d_out, out, to_coeffs ? b_coef : b_vals);
    if (int rc = ragged_wait_last(ctx)) return rc;
    if (int rc = st.upload()) return rc;
    const size_t b_so = sizeof(int64_t) * so.size();
    MTG_HIP_TRY(ctx, ensure(&ctx->ragged, &ctx->ragged_bytes, align_up(b_so)));
    if (int rc = ragged_upload(ctx, b_so, ctx->ragged, [&](void* p) { std::memcpy(p, so.data(), b_so); })) return rc;
    MTG_HIP_TRY(ctx, time_begin(ctx));
    MTG_HIP_TRY(ctx, mtg::launch_vertex_map_ragged(to_coeffs, N, d_in, d_times, static_cast<const int64_t*>(ctx->ragged),
                                                   d_out, batch, so.back(), D, ctx->stream));
    MTG_HIP_TRY(ctx, time_end(ctx));
    if (int rc = ragged_mark_last(ctx)) return rc;
    return st.finish();
  } catch (const std::bad_alloc&) {
    return set_error(ctx, MTG_ERR_OUT_OF_MEMORY, "ragged vertex map: out of host memory");
  }
}

}  // namespace

int mtg_coefficients_from_vertices_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                                const double* vertex_values, const double* times, double* coeffs,
                                                unsigned flags) {
  return run_vertex_map_ragged(ctx, true, N, D, batch, seg_count, vertex_values, times, coeffs, flags);
}

int mtg_vertex_derivatives_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                        const double* coeffs, const double* times, double* vertex_values,
                                        unsigned flags) {
  return run_vertex_map_ragged(ctx, false, N, D, batch, seg_count, coeffs, times, vertex_values, flags);
}

int mtg_vertex_ragged_tile(int N, int D) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (D < 1) return MTG_ERR_SIZE_MISMATCH;
  const int ts = mtg::vertex_ragged_tile(N, D);
  return ts < 1 ? MTG_ERR_TOO_LARGE : ts;
}

int mtg_min_max_magnitude_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* coeffs,
                                const double* times, int derivative, uint32_t dimension_mask,
                                mtg_extremum* minimum, mtg_extremum* maximum, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_order(ctx, N)) return rc;
  if (int rc = check_dims(ctx, D, K, batch)) return rc;
  if (K > 256) return set_error(ctx, MTG_ERR_TOO_LARGE, "K must be <= 256");
  if (derivative < 0 || derivative > N - 2)
    return set_error(ctx, MTG_ERR_BAD_DERIVATIVE, "derivative must be in [0, N-2] (polynomial.cpp:62-65)");
  const uint32_t all = D >= 32 ? 0xffffffffu : ((1u << D) - 1u);
  const uint32_t dims = dimension_mask ? dimension_mask : all;
  if (D > 32 || (dims & ~all)) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "dimension_mask out of range");
  if (batch == 0) return MTG_OK;
  if (!coeffs || !times) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "coeffs and times are required");
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nB = (size_t)batch;
  const double *d_coef, *d_times;
  mtg_extremum *d_min, *d_max;
  Staged st(ctx, flags);
  st.in(&d_coef, coeffs, sizeof(double) * nB * K * D * N);
  st.in(&d_times, times, sizeof(double) * nB * K);
  st.out(&d_min, minimum, sizeof(mtg_extremum) * nB);
  st.out(&d_max, maximum, sizeof(mtg_extremum) * nB);
  if (int rc = st.upload()) return rc;
  MTG_HIP_TRY(ctx, time_begin(ctx));
  MTG_HIP_TRY(ctx, mtg::launch_min_max_magnitude(N, d_coef, d_times, batch, K, D, derivative, dims, d_min, d_max,
                                                 ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  return st.finish();
}

int mtg_min_max_magnitude_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                       const double* coeffs, const double* times, int derivative,
                                       uint32_t dimension_mask, mtg_extremum* minimum, mtg_extremum* maximum,
                                       unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_order(ctx, N)) return rc;
  if (D < 1 || batch < 0) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need D >= 1, batch >= 0");
  if (derivative < 0 || derivative > N - 2)
    return set_error(ctx, MTG_ERR_BAD_DERIVATIVE, "derivative must be in [0, N-2] (polynomial.cpp:62-65)");
  const uint32_t all = D >= 32 ? 0xffffffffu : ((1u << D) - 1u);
  const uint32_t dims = dimension_mask ? dimension_mask : all;
  if (D > 32 || (dims & ~all)) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "dimension_mask out of range");
  if (batch == 0) return MTG_OK;
  if (!seg_count) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "seg_count is required (a host array)");
  try {
    mtg::RaggedPlan plan;
    if (mtg::ragged_plan(batch, seg_count, &plan) != MTG_OK)
      return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "every seg_count must be >= 1");
    if (plan.groups.back().K > 256) return set_error(ctx, MTG_ERR_TOO_LARGE, "every seg_count must be <= 256");
    if (!coeffs || !times) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "coeffs and times are required");
    std::lock_guard<std::mutex> g(ctx->mu);
    return run_min_max_ragged(ctx, N, D, plan, coeffs, times, derivative, dims, minimum, maximum, flags);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, MTG_ERR_OUT_OF_MEMORY, "ragged min / max magnitude: out of host memory");
  }
}

namespace {

// Body of mtg_segment_min_max_magnitude_batch / mtg_segment_min_max_axis_batch: one launch over the
// items (segments, or (segment, dimension) pairs), nothing else.
int run_segment_extrema(mtg_ctx* ctx, bool axis, int N, int D, int64_t S, const double* coeffs, const double* times,
                        const double* windows, int derivative, uint32_t dimension_mask, mtg_extremum* minimum,
                        mtg_extremum* maximum, double* candidate_times, int32_t* candidate_count,
                        int candidate_capacity, int32_t* status, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_order(ctx, N)) return rc;
  if (int rc = check_dims(ctx, D, 1, S)) return rc;
  if (derivative < 0 || derivative > N - 2)
    return set_error(ctx, MTG_ERR_BAD_DERIVATIVE, "derivative must be in [0, N-2] (polynomial.cpp:62-65)");
  const uint32_t all = D >= 32 ? 0xffffffffu : ((1u << D) - 1u);
  const uint32_t dims = dimension_mask ? dimension_mask : all;
  if (D > 32 || (dims & ~all)) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "dimension_mask out of range");
  if (candidate_times && candidate_capacity < 2)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "candidate_capacity must be >= 2 (the two ends)");
  if (S == 0) return MTG_OK;
  if (!coeffs || (!times && !windows))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "coeffs and times (or windows) are required");
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nS = (size_t)S, nI = axis ? nS * D : nS, cap = candidate_times ? (size_t)candidate_capacity : 0;
  const double *d_coef, *d_times, *d_win;
  mtg_extremum *d_min, *d_max;
  double* d_cand;
  int32_t *d_count, *d_status;
  Staged st(ctx, flags);
  st.in(&d_coef, coeffs, sizeof(double) * nS * D * N);
  st.in(&d_times, times, sizeof(double) * nS);
  st.in(&d_win, windows, sizeof(double) * nS * 2);
  st.out(&d_min, minimum, sizeof(mtg_extremum) * nI);
  st.out(&d_max, maximum, sizeof(mtg_extremum) * nI);
  st.out(&d_cand, candidate_times, sizeof(double) * nI * cap);
  st.out(&d_count, candidate_count, sizeof(int32_t) * nI);
  st.out(&d_status, status, sizeof(int32_t) * nS);
  if (int rc = st.upload()) return rc;
  MTG_HIP_TRY(ctx, time_begin(ctx));
  MTG_HIP_TRY(ctx, mtg::launch_segment_extrema(axis, N, d_coef, d_times, d_win, S, D, derivative, dims, d_min, d_max,
                                               d_cand, d_count, candidate_capacity, d_status, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  return st.finish();
}

}  // namespace

int mtg_segment_min_max_magnitude_batch(mtg_ctx* ctx, int N, int D, int64_t n_segments, const double* coeffs,
                                        const double* times, const double* windows, int derivative,
                                        uint32_t dimension_mask, mtg_extremum* minimum, mtg_extremum* maximum,
                                        double* candidate_times, int32_t* candidate_count, int candidate_capacity,
                                        int32_t* status, unsigned flags) {
  return run_segment_extrema(ctx, false, N, D, n_segments, coeffs, times, windows, derivative, dimension_mask, minimum,
                             maximum, candidate_times, candidate_count, candidate_capacity, status, flags);
}

int mtg_segment_min_max_axis_batch(mtg_ctx* ctx, int N, int D, int64_t n_segments, const double* coeffs,
                                   const double* times, const double* windows, int derivative, mtg_extremum* minimum,
                                   mtg_extremum* maximum, double* candidate_times, int32_t* candidate_count,
                                   int candidate_capacity, int32_t* status, unsigned flags) {
  return run_segment_extrema(ctx, true, N, D, n_segments, coeffs, times, windows, derivative, 0, minimum, maximum,
                             candidate_times, candidate_count, candidate_capacity, status, flags);
}

int mtg_evaluate_at_path(int N, int D, int K, int64_t M, int n_derivatives) {
  if (int rc = check_order(nullptr, N)) return rc;
  if (int rc = check_dims(nullptr, D, K, M)) return rc;
  if (n_derivatives < 1 || n_derivatives > N) return MTG_ERR_BAD_DERIVATIVE;
  mtg::EvalAtPlan plan;
  return mtg::evaluate_at_plan(N, D, K, M, n_derivatives, &plan) ? plan.path : MTG_ERR_TOO_LARGE;
}

int mtg_evaluate_at_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* coeffs,
                          const double* times, const double* t_query, int64_t t_stride, int64_t M,
                          int derivative_begin, int n_derivatives, double* out, uint8_t* in_range_out,
                          int32_t* status, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_order(ctx, N)) return rc;
  if (int rc = check_dims(ctx, D, K, batch)) return rc;
  if (M < 0) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need M >= 0");
  if (derivative_begin < 0 || n_derivatives < 1 || n_derivatives > N)
    return set_error(ctx, MTG_ERR_BAD_DERIVATIVE, "need derivative_begin >= 0 and n_derivatives in [1, N]");
  if (t_stride < 0 || (t_stride > 0 && t_stride < M))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "t_stride must be 0 (shared query times) or >= M");
  mtg::EvalAtPlan plan;
  if (!mtg::evaluate_at_plan(N, D, K, M, n_derivatives, &plan))
    return set_error(ctx, MTG_ERR_TOO_LARGE, "a block's rows exceed LDS (n_derivatives * D > 128)");
  if (batch == 0 || M == 0) return MTG_OK;
  if (!coeffs || !times || !t_query || !out)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "coeffs, times, t_query and out are required");
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nB = (size_t)batch, nM = (size_t)M;
  const double *d_coef, *d_times, *d_tq;
  double* d_out;
  uint8_t* d_in;
  int32_t* d_status;
  Staged st(ctx, flags);
  st.in(&d_coef, coeffs, sizeof(double) * nB * K * D * N);
  st.in(&d_times, times, sizeof(double) * nB * K);
  st.in(&d_tq, t_query, sizeof(double) * (t_stride ? (nB - 1) * (size_t)t_stride + nM : nM));
  st.out(&d_out, out, sizeof(double) * nB * nM * n_derivatives * D);
  st.out(&d_in, in_range_out, nB * nM);
  st.out(&d_status, status, sizeof(int32_t) * nB);
  if (int rc = st.upload()) return rc;
  MTG_HIP_TRY(ctx, time_begin(ctx));
  MTG_HIP_TRY(ctx, mtg::launch_evaluate_at(N, D, K, batch, d_coef, d_times, d_tq, t_stride, M, derivative_begin,
                                           n_derivatives, d_out, d_in, d_status, ctx->stream));
  MTG_HIP_TRY(ctx, time_end(ctx));
  return st.finish();
}

int mtg_evaluate_at_ragged_path(int N, int D, int K_max, int64_t M, int n_derivatives) {
  return mtg_evaluate_at_path(N, D, K_max, M, n_derivatives);
}

int mtg_evaluate_at_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                 const double* coeffs, const double* times, const double* t_query, int64_t t_stride,
                                 int64_t M, int derivative_begin, int n_derivatives, double* out,
                                 uint8_t* in_range_out, int32_t* status, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_order(ctx, N)) return rc;
  if (D < 1 || batch < 0) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need D >= 1, batch >= 0");
  if (M < 0) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need M >= 0");
  if (derivative_begin < 0 || n_derivatives < 1 || n_derivatives > N)
    return set_error(ctx, MTG_ERR_BAD_DERIVATIVE, "need derivative_begin >= 0 and n_derivatives in [1, N]");
  if (t_stride < 0 || (t_stride > 0 && t_stride < M))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "t_stride must be 0 (shared query times) or >= M");
  int k_max = 0;
  try {
    std::vector<int64_t> so;
    if (int rc = ragged_check_counts(ctx, batch, seg_count, &k_max, &so)) return rc;
    mtg::EvalAtPlan plan;
    if (!mtg::evaluate_at_plan(N, D, std::max(k_max, 1), M, n_derivatives, &plan))
      return set_error(ctx, MTG_ERR_TOO_LARGE, "a block's rows exceed LDS (n_derivatives * D > 128)");
    if (batch == 0 || M == 0) return MTG_OK;
    if (!coeffs || !times || !t_query || !out)
      return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "coeffs, times, t_query and out are required");
    std::lock_guard<std::mutex> g(ctx->mu);
    return run_evaluate_at_ragged(ctx, N, D, k_max, so, coeffs, times, t_query, t_stride, M, derivative_begin,
                                  n_derivatives, out, in_range_out, status, flags);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, MTG_ERR_OUT_OF_MEMORY, "ragged evaluate: out of host memory");
  }
}

namespace {

// What the uniform and the CSR form of evaluateRange differ in: the shape of coeffs and times, and
// with it the three launches.  Everything else -- staging, the two-call and the one-call protocol,
// offsets, capacity -- is one body (run_evaluate_range, run_evaluate_range_full).
struct EvalShape {
  int K;        // the segment count; CSR: the largest K_b
  size_t nseg;  // segments of the whole batch: coeffs [nseg][D][N], times [nseg]
  const std::vector<int64_t>* so = nullptr;  // CSR: the segment offsets [batch + 1] (host); uniform: null
  mtg::EvalRagged rag{};                     // CSR: their device copy and the clock's staging rule (eval_shape_begin)
};

// CSR: the segment offsets to ctx->ragged (mtg_evaluate_at_ragged_batch's mechanism: the only bytes
// the call makes on the host and uploads besides the caller's arrays), before the first launch.
int eval_shape_begin(mtg_ctx* ctx, EvalShape* s) {
  if (!s->so) return MTG_OK;
  if (int rc = ragged_wait_last(ctx)) return rc;
  const size_t b_so = sizeof(int64_t) * s->so->size();
  MTG_HIP_TRY(ctx, ensure(&ctx->ragged, &ctx->ragged_bytes, align_up(b_so)));
  if (int rc = ragged_upload(ctx, b_so, ctx->ragged, [&](void* p) { std::memcpy(p, s->so->data(), b_so); })) return rc;
  s->rag.seg_off = static_cast<const int64_t*>(ctx->ragged);
  s->rag.K_max = s->K;
  s->rag.clock_slice = mtg::eval_ragged_clock_slice(s->so->data(), (int64_t)s->so->size() - 1);
  return MTG_OK;
}

// CSR: after the call's last launch (the next ragged call may run on another stream)
int eval_shape_end(mtg_ctx* ctx, const EvalShape& s) { return s.so ? ragged_mark_last(ctx) : MTG_OK; }

hipError_t eval_count(const EvalShape& s, int N, int D, int64_t B, const double* times, double t_start, double t_end,
                      double dt, int64_t* counts, hipStream_t stream) {
  return s.so ? mtg::launch_eval_count_ragged(s.rag, B, times, t_start, t_end, dt, counts, stream)
              : mtg::launch_eval_count(N, D, s.K, B, times, t_start, t_end, dt, counts, stream);
}

hipError_t eval_runs_counts(const EvalShape& s, int64_t B, const double* times, double t_start, double t_end, double dt,
                            int64_t* counts, int64_t* offsets, void* ws, int cap, int64_t* total, hipStream_t stream) {
  return s.so ? mtg::launch_eval_runs_counts_ragged(s.rag, B, times, t_start, t_end, dt, counts, offsets, ws, cap, total,
                                                    stream)
              : mtg::launch_eval_runs_counts(s.K, B, times, t_start, t_end, dt, counts, offsets, ws, cap, total, stream);
}

hipError_t eval_range(const EvalShape& s, int N, int D, int64_t B, const double* coeffs, const double* times,
                      double t_start, double t_end, double dt, int derivative, const int64_t* counts,
                      const int64_t* offsets, double* out, double* sample_times, void* ws, int cap, hipStream_t stream,
                      bool runs_ready = false, int64_t* offsets_out = nullptr, int64_t capacity = INT64_MAX,
                      const int64_t* total = nullptr) {
  return s.so ? mtg::launch_eval_range_ragged(N, D, s.rag, B, coeffs, times, t_start, t_end, dt, derivative, counts,
                                              offsets, out, sample_times, ws, cap, stream, runs_ready, offsets_out,
                                              capacity, total)
              : mtg::launch_eval_range(N, D, s.K, B, coeffs, times, t_start, t_end, dt, derivative, counts, offsets, out,
                                       sample_times, ws, cap, stream, runs_ready, offsets_out, capacity, total);
}

// Body of mtg_evaluate_range_batch and mtg_evaluate_range_ragged_batch, after their argument checks
// (batch > 0), under ctx->mu.
int run_evaluate_range(mtg_ctx* ctx, int N, int D, EvalShape& sh, int64_t batch, const double* coeffs,
                       const double* times, double t_start, double t_end, double dt, int derivative, int64_t* counts,
                       const int64_t* offsets, double* out, double* sample_times, unsigned flags) {
  const int K = sh.K;
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = eval_shape_begin(ctx, &sh)) return rc;
  const bool dev = flags & MTG_FLAG_DEVICE_PTRS;
  if (dev) {
    if (!out) {
      MTG_HIP_TRY(ctx, eval_count(sh, N, D, batch, times, t_start, t_end, dt, counts, ctx->stream));
    } else {
      int cap = 0;
      const size_t wsb = mtg::eval_workspace_bytes(K, batch, &cap);
      MTG_HIP_TRY(ctx, ensure(&ctx->workspace, &ctx->workspace_bytes, std::max<size_t>(wsb, 256)));
      MTG_HIP_TRY(ctx, time_begin(ctx, false));  // two kernels: the run table, then the samples
      MTG_HIP_TRY(ctx, eval_range(sh, N, D, batch, coeffs, times, t_start, t_end, dt, derivative, counts, offsets, out,
                                  sample_times, ctx->workspace, cap, ctx->stream));
      MTG_HIP_TRY(ctx, time_end(ctx));
    }
    if (int rc = eval_shape_end(ctx, sh)) return rc;
    if (!(flags & MTG_FLAG_ASYNC)) MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MTG_OK;
  }
  // Host pointers: stage everything.
  const size_t b_times = sizeof(double) * sh.nseg;
  const size_t b_coeffs = coeffs ? sizeof(double) * sh.nseg * D * N : 0;
  const size_t b_counts = sizeof(int64_t) * (size_t)batch;
  int64_t total = 0;
  if (out) {
    for (int64_t b = 0; b < batch; ++b) total = std::max<int64_t>(total, offsets[b] + counts[b]);
  }
  const size_t b_out = out ? sizeof(double) * (size_t)total * D : 0;
  const size_t b_st = (out && sample_times) ? sizeof(double) * (size_t)total : 0;
  size_t off = 0;
  const size_t o_times = off; off = align_up(off + b_times);
  const size_t o_coeffs = off; off = align_up(off + b_coeffs);
  const size_t o_counts = off; off = align_up(off + b_counts);
  const size_t o_offsets = off; off = align_up(off + b_counts);
  const size_t o_out = off; off = align_up(off + b_out);
  const size_t o_st = off; off = align_up(off + b_st);
  MTG_HIP_TRY(ctx, ensure(&ctx->staging, &ctx->staging_bytes, std::max<size_t>(off, 256)));
  char* base = static_cast<char*>(ctx->staging);
  MTG_HIP_TRY(ctx, hipMemcpyAsync(base + o_times, times, b_times, hipMemcpyHostToDevice, ctx->stream));
  if (!out) {
    MTG_HIP_TRY(ctx, eval_count(sh, N, D, batch, reinterpret_cast<double*>(base + o_times), t_start, t_end, dt,
                                reinterpret_cast<int64_t*>(base + o_counts), ctx->stream));
    MTG_HIP_TRY(ctx, hipMemcpyAsync(counts, base + o_counts, b_counts, hipMemcpyDeviceToHost, ctx->stream));
  } else {
    MTG_HIP_TRY(ctx, hipMemcpyAsync(base + o_coeffs, coeffs, b_coeffs, hipMemcpyHostToDevice, ctx->stream));
    MTG_HIP_TRY(ctx, hipMemcpyAsync(base + o_offsets, offsets, b_counts, hipMemcpyHostToDevice, ctx->stream));
    MTG_HIP_TRY(ctx, hipMemcpyAsync(base + o_counts, counts, b_counts, hipMemcpyHostToDevice, ctx->stream));
    int cap = 0;
    const size_t wsb = mtg::eval_workspace_bytes(K, batch, &cap);
    MTG_HIP_TRY(ctx, ensure(&ctx->workspace, &ctx->workspace_bytes, std::max<size_t>(wsb, 256)));
    MTG_HIP_TRY(ctx, time_begin(ctx, false));
    MTG_HIP_TRY(ctx, eval_range(sh, N, D, batch, reinterpret_cast<double*>(base + o_coeffs),
                                reinterpret_cast<double*>(base + o_times), t_start, t_end, dt, derivative,
                                reinterpret_cast<int64_t*>(base + o_counts),
                                reinterpret_cast<int64_t*>(base + o_offsets), reinterpret_cast<double*>(base + o_out),
                                sample_times ? reinterpret_cast<double*>(base + o_st) : nullptr, ctx->workspace, cap,
                                ctx->stream));
    MTG_HIP_TRY(ctx, time_end(ctx));
    MTG_HIP_TRY(ctx, hipMemcpyAsync(out, base + o_out, b_out, hipMemcpyDeviceToHost, ctx->stream));
    if (sample_times) MTG_HIP_TRY(ctx, hipMemcpyAsync(sample_times, base + o_st, b_st, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (int rc = eval_shape_end(ctx, sh)) return rc;
  MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MTG_OK;
}

// Body of mtg_evaluate_range_batch_full and mtg_evaluate_range_ragged_batch_full, after their argument
// checks, under ctx->mu.
int run_evaluate_range_full(mtg_ctx* ctx, int N, int D, EvalShape& sh, int64_t batch, const double* coeffs,
                            const double* times, double t_start, double t_end, double dt, int derivative,
                            int64_t* counts, int64_t* offsets, int64_t* total, double* out, double* sample_times,
                            int64_t capacity, unsigned flags) {
  const int K = sh.K;
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool dev = flags & MTG_FLAG_DEVICE_PTRS;
  if (batch == 0) {
    if (dev) MTG_HIP_TRY(ctx, hipMemsetAsync(total, 0, sizeof(int64_t), ctx->stream));
    else *total = 0;
    return MTG_OK;
  }
  if (int rc = eval_shape_begin(ctx, &sh)) return rc;
  int cap = 0;
  const size_t wsb = mtg::eval_full_workspace_bytes(K, batch, &cap);
  MTG_HIP_TRY(ctx, ensure(&ctx->workspace, &ctx->workspace_bytes, std::max<size_t>(wsb, 256)));
  int64_t* d_total_ws = reinterpret_cast<int64_t*>(static_cast<char*>(ctx->workspace) + wsb - sizeof(int64_t));
  if (dev) {
    // counts, offsets (in-block prefix, then final) and the total, then the samples: four kernels on
    // the stream, no host round trip in between
    MTG_HIP_TRY(ctx, time_begin(ctx, false));
    MTG_HIP_TRY(ctx, eval_runs_counts(sh, batch, times, t_start, t_end, dt, counts, offsets, ctx->workspace, cap, total,
                                      ctx->stream));
    MTG_HIP_TRY(ctx, eval_range(sh, N, D, batch, coeffs, times, t_start, t_end, dt, derivative, counts, offsets, out,
                                sample_times, ctx->workspace, cap, ctx->stream, true, offsets, capacity, total));
    MTG_HIP_TRY(ctx, time_end(ctx));
    if (int rc = eval_shape_end(ctx, sh)) return rc;
    if (flags & MTG_FLAG_ASYNC) return MTG_OK;
    int64_t tot = 0;
    MTG_HIP_TRY(ctx, hipMemcpyAsync(&tot, total, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (tot > capacity) {
      char buf[160];
      snprintf(buf, sizeof(buf), "evaluateRange needs %lld samples, capacity is %lld",
               (long long)tot, (long long)capacity);
      return set_error(ctx, MTG_ERR_TOO_LARGE, buf);
    }
    return MTG_OK;
  }
  // host arrays: counts and offsets first (one 8-B read of the total sizes the staging), then the
  // samples straight into staging sized to the total
  const size_t b_coef = sizeof(double) * (size_t)batch * K * D * N, b_times = sizeof(double) * (size_t)batch * K,
               b_cnt = sizeof(int64_t) * (size_t)batch;
  size_t off = 0;
  const size_t o_times = off; off = align_up(off + b_times);
  const size_t o_coef = off; off = align_up(off + b_coef);
  const size_t o_cnt = off; off = align_up(off + b_cnt);
  const size_t o_offs = off; off = align_up(off + b_cnt);
  const size_t in_end = off;
  MTG_HIP_TRY(ctx, ensure(&ctx->staging, &ctx->staging_bytes, std::max<size_t>(in_end, 256)));
  char* base = static_cast<char*>(ctx->staging);
  MTG_HIP_TRY(ctx, hipMemcpyAsync(base + o_times, times, b_times, hipMemcpyHostToDevice, ctx->stream));
  MTG_HIP_TRY(ctx, hipMemcpyAsync(base + o_coef, coeffs, b_coef, hipMemcpyHostToDevice, ctx->stream));
  int64_t* d_cnt = reinterpret_cast<int64_t*>(base + o_cnt);
  int64_t* d_offs = reinterpret_cast<int64_t*>(base + o_offs);
  MTG_HIP_TRY(ctx, time_begin(ctx, false));
  MTG_HIP_TRY(ctx, eval_runs_counts(sh, batch, reinterpret_cast<const double*>(base + o_times), t_start, t_end, dt,
                                    d_cnt, d_offs, ctx->workspace, cap, d_total_ws, ctx->stream));
  int64_t tot = 0;
  MTG_HIP_TRY(ctx, hipMemcpyAsync(&tot, d_total_ws, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *total = tot;
  const size_t b_out = sizeof(double) * (size_t)(tot <= capacity ? tot : 0) * D;
  const size_t b_st = sample_times ? sizeof(double) * (size_t)(tot <= capacity ? tot : 0) : 0;
  const size_t o_out = in_end, o_st = align_up(o_out + b_out), all_end = align_up(o_st + b_st);
  if (all_end > ctx->staging_bytes) {  // grow, keeping the staged inputs and counts
    void* grown = nullptr;
    MTG_HIP_TRY(ctx, hipMalloc(&grown, all_end));
    MTG_HIP_TRY(ctx, hipMemcpyAsync(grown, ctx->staging, in_end, hipMemcpyDeviceToDevice, ctx->stream));
    MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    MTG_HIP_TRY(ctx, hipFree(ctx->staging));
    ctx->staging = grown;
    ctx->staging_bytes = all_end;
    base = static_cast<char*>(grown);
    d_cnt = reinterpret_cast<int64_t*>(base + o_cnt);
    d_offs = reinterpret_cast<int64_t*>(base + o_offs);
  }
  if (tot > capacity) {  // counts, final offsets and the total for the caller's retry; no samples
    MTG_HIP_TRY(ctx, eval_range(sh, N, D, batch, reinterpret_cast<const double*>(base + o_coef),
                                reinterpret_cast<const double*>(base + o_times), t_start, t_end, dt, derivative, d_cnt,
                                d_offs, nullptr, nullptr, ctx->workspace, cap, ctx->stream, true, d_offs, 0));
    MTG_HIP_TRY(ctx, time_end(ctx));
    if (int rc = eval_shape_end(ctx, sh)) return rc;
    MTG_HIP_TRY(ctx, hipMemcpyAsync(counts, d_cnt, b_cnt, hipMemcpyDeviceToHost, ctx->stream));
    MTG_HIP_TRY(ctx, hipMemcpyAsync(offsets, d_offs, b_cnt, hipMemcpyDeviceToHost, ctx->stream));
    MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    char buf[160];
    snprintf(buf, sizeof(buf), "evaluateRange needs %lld samples, capacity is %lld", (long long)tot,
             (long long)capacity);
    return set_error(ctx, MTG_ERR_TOO_LARGE, buf);
  }
  MTG_HIP_TRY(ctx, eval_range(sh, N, D, batch, reinterpret_cast<const double*>(base + o_coef),
                              reinterpret_cast<const double*>(base + o_times), t_start, t_end, dt, derivative, d_cnt,
                              d_offs, reinterpret_cast<double*>(base + o_out),
                              sample_times ? reinterpret_cast<double*>(base + o_st) : nullptr, ctx->workspace, cap,
                              ctx->stream, true, d_offs, capacity));
  MTG_HIP_TRY(ctx, time_end(ctx));
  if (int rc = eval_shape_end(ctx, sh)) return rc;
  MTG_HIP_TRY(ctx, hipMemcpyAsync(counts, d_cnt, b_cnt, hipMemcpyDeviceToHost, ctx->stream));
  MTG_HIP_TRY(ctx, hipMemcpyAsync(offsets, d_offs, b_cnt, hipMemcpyDeviceToHost, ctx->stream));
  if (b_out) MTG_HIP_TRY(ctx, hipMemcpyAsync(out, base + o_out, b_out, hipMemcpyDeviceToHost, ctx->stream));
  if (b_st) MTG_HIP_TRY(ctx, hipMemcpyAsync(sample_times, base + o_st, b_st, hipMemcpyDeviceToHost, ctx->stream));
  MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MTG_OK;
}

// The checks the two CSR evaluateRange entries share after their own on N, D, batch and capacity: dt
// and derivative, then seg_count (ragged_check_counts), then -- for a call that writes samples -- the
// sample kernels' LDS at the largest K_b, with the result of the uniform call at that K and its HIP
// error text in the message.  All before any device work.
int eval_ragged_check(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count, double dt, int derivative,
                      bool samples, int* k_max, std::vector<int64_t>* so) {
  if (!(dt > 0.0) || derivative < 0)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "dt must be > 0 and derivative >= 0");
  if (int rc = ragged_check_counts(ctx, batch, seg_count, k_max, so)) return rc;
  if (batch > 0 && samples) MTG_HIP_TRY(ctx, mtg::eval_range_lds_check(N, D, *k_max));
  return MTG_OK;
}

}  // namespace

int mtg_evaluate_range_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch,
                             const double* coeffs, const double* times, double t_start,
                             double t_end, double dt, int derivative, int64_t* counts,
                             const int64_t* offsets, double* out, double* sample_times,
                             unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_order(ctx, N)) return rc;
  if (int rc = check_dims(ctx, D, K, batch)) return rc;
  if (!(dt > 0.0) || derivative < 0)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "dt must be > 0 and derivative >= 0");
  if (batch == 0) return MTG_OK;
  if (!times || !counts || (out && (!coeffs || !offsets)))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "times and counts required; out needs coeffs and offsets");
  std::lock_guard<std::mutex> g(ctx->mu);
  EvalShape sh{K, (size_t)batch * K};
  return run_evaluate_range(ctx, N, D, sh, batch, coeffs, times, t_start, t_end, dt, derivative, counts, offsets, out,
                            sample_times, flags);
}

int mtg_evaluate_range_batch_full(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* coeffs,
                                  const double* times, double t_start, double t_end, double dt, int derivative,
                                  int64_t* counts, int64_t* offsets, int64_t* total, double* out,
                                  double* sample_times, int64_t capacity, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_order(ctx, N)) return rc;
  if (K < 1 || D < 1 || batch < 0 || capacity < 0)
    return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need K >= 1, D >= 1, batch >= 0, capacity >= 0");
  if (!(dt > 0.0) || derivative < 0)
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "dt must be > 0 and derivative >= 0");
  if (!coeffs || !times || !counts || !offsets || !total || (capacity > 0 && !out))
    return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "coeffs, times, counts, offsets, total and out are required");
  std::lock_guard<std::mutex> g(ctx->mu);
  EvalShape sh{K, (size_t)batch * K};
  return run_evaluate_range_full(ctx, N, D, sh, batch, coeffs, times, t_start, t_end, dt, derivative, counts, offsets,
                                 total, out, sample_times, capacity, flags);
}

int mtg_evaluate_range_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                    const double* coeffs, const double* times, double t_start, double t_end,
                                    double dt, int derivative, int64_t* counts, const int64_t* offsets, double* out,
                                    double* sample_times, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_order(ctx, N)) return rc;
  if (D < 1 || batch < 0) return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need D >= 1, batch >= 0");
  try {
    int k_max = 0;
    std::vector<int64_t> so;
    if (int rc = eval_ragged_check(ctx, N, D, batch, seg_count, dt, derivative, out != nullptr, &k_max, &so)) return rc;
    if (batch == 0) return MTG_OK;
    if (!times || !counts || (out && (!coeffs || !offsets)))
      return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "times and counts required; out needs coeffs and offsets");
    std::lock_guard<std::mutex> g(ctx->mu);
    EvalShape sh{k_max, (size_t)so.back(), &so};
    return run_evaluate_range(ctx, N, D, sh, batch, coeffs, times, t_start, t_end, dt, derivative, counts, offsets, out,
                              sample_times, flags);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, MTG_ERR_OUT_OF_MEMORY, "ragged evaluateRange: out of host memory");
  }
}

int mtg_evaluate_range_ragged_batch_full(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                         const double* coeffs, const double* times, double t_start, double t_end,
                                         double dt, int derivative, int64_t* counts, int64_t* offsets, int64_t* total,
                                         double* out, double* sample_times, int64_t capacity, unsigned flags) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (int rc = check_order(ctx, N)) return rc;
  if (D < 1 || batch < 0 || capacity < 0)
    return set_error(ctx, MTG_ERR_SIZE_MISMATCH, "need D >= 1, batch >= 0, capacity >= 0");
  try {
    int k_max = 0;
    std::vector<int64_t> so;
    if (int rc = eval_ragged_check(ctx, N, D, batch, seg_count, dt, derivative, true, &k_max, &so)) return rc;
    if (batch == 0 && !total) return MTG_OK;
    if (batch > 0 && (!coeffs || !times || !counts || !offsets || !total || (capacity > 0 && !out)))
      return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "coeffs, times, counts, offsets, total and out are required");
    std::lock_guard<std::mutex> g(ctx->mu);
    EvalShape sh{std::max(k_max, 1), batch ? (size_t)so.back() : 0, &so};
    return run_evaluate_range_full(ctx, N, D, sh, batch, coeffs, times, t_start, t_end, dt, derivative, counts, offsets,
                                   total, out, sample_times, capacity, flags);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, MTG_ERR_OUT_OF_MEMORY, "ragged evaluateRange: out of host memory");
  }
}

int mtg_last_kernel_ms(mtg_ctx* ctx, float* ms) {
  if (!ms) return MTG_ERR_INVALID_ARGUMENT;
  int n = 0;
  int rc = mtg_kernel_times(ctx, ms, 1, &n);
  if (rc == MTG_OK && n == 0) return set_error(ctx, MTG_ERR_INVALID_ARGUMENT, "no timed launch yet");
  return rc;
}

int mtg_enable_timing(mtg_ctx* ctx, int ring) {
  if (!ctx || ring < 0) return MTG_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  MTG_HIP_TRY(ctx, create_events(ctx, ring));
  return MTG_OK;
}

int mtg_kernel_times(mtg_ctx* ctx, float* ms, int n, int* n_out) {
  if (!ctx || !ms || n < 0 || !n_out) return MTG_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int64_t ring = (int64_t)ctx->ev_start.size();
  const int64_t have = std::min<int64_t>(ctx->launches, ring);
  const int64_t take = std::min<int64_t>(have, n);
  *n_out = 0;
  if (take == 0) return MTG_OK;
  const size_t newest = (size_t)((ctx->launches - 1) % ring);
  MTG_HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop[newest]));
  for (int64_t i = 0; i < take; ++i) {
    const size_t slot = (size_t)((ctx->launches - take + i) % ring);
    MTG_HIP_TRY(ctx, hipEventElapsedTime(&ms[i], ctx->ev_start[slot], ctx->ev_stop[slot]));
  }
  *n_out = (int)take;
  return MTG_OK;
}

}  // extern "C"
