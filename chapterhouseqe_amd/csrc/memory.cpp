// memory.cpp -- the error mapping of HIP calls, the HBM and host memory pools, a context's auxiliary streams and kernel-time
// events, the host worker pool and the phase timer.
#include "engine.hpp"

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <thread>

namespace chq {

void check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    int code = (e == hipErrorOutOfMemory) ? CHQ_ERR_OUT_OF_MEMORY : CHQ_ERR_DEVICE;
    throw ChqError{code, std::string(what) + ": " + hipGetErrorString(e)};
  }
}

// =================================================================================================
// memory
// =================================================================================================
DevicePool& DevicePool::instance() {
  static DevicePool* pool = new DevicePool();   // intentionally leaked: must outlive late Arrow releases
  return *pool;
}
static size_t size_class(size_t bytes) {
  if (bytes < 256) return 256;
  if (bytes <= (1u << 20)) { size_t c = 256; while (c < bytes) c <<= 1; return c; }
  const size_t g = 2u << 20;
  return (bytes + g - 1) / g * g;
}
static uint64_t pool_key(size_t cap, int device) { return ((uint64_t)cap << 8) | (uint64_t)(device & 0xff); }
void* DevicePool::alloc(size_t bytes, int device, size_t* cap_out) {
  const size_t cap = size_class(bytes);
  *cap_out = cap;
  {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = free_.find(pool_key(cap, device));
    if (it != free_.end() && !it->second.empty()) { void* p = it->second.back(); it->second.pop_back(); return p; }
  }
  // allocate on the device the block is keyed by, whatever the calling thread's current device is (peer copies
  // allocate on the destination GPU from a call that started on the source context)
  int current = device;
  (void)hipGetDevice(&current);
  if (current != device) check_hip(hipSetDevice(device), "hipSetDevice");
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, cap);
  if (e == hipErrorOutOfMemory) { trim(); e = hipMalloc(&p, cap); }
  if (current != device) (void)hipSetDevice(current);
  check_hip(e, "hipMalloc");
  return p;
}
void DevicePool::free(void* p, size_t cap, int device) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(mu_);
  free_[pool_key(cap, device)].push_back(p);
}
void DevicePool::trim() {
  std::unordered_map<uint64_t, std::vector<void*>> f;
  { std::lock_guard<std::mutex> lk(mu_); f.swap(free_); }
  for (auto& kv : f) for (void* p : kv.second) (void)hipFree(p);
}

HostPool& HostPool::instance() {
  static HostPool* pool = new HostPool();   // leaked on purpose, like the device pool
  return *pool;
}
void* HostPool::alloc(size_t bytes, size_t* cap_out) {
  const size_t cap = size_class(bytes < 64 ? 64 : bytes);
  *cap_out = cap;
  if (cap >= ((size_t)1 << 20)) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = free_.find(cap);
    if (it != free_.end() && !it->second.empty()) { void* p = it->second.back(); it->second.pop_back(); cached_ -= cap; return p; }
  }
  void* p = nullptr;
  if (posix_memalign(&p, 64, cap) != 0) throw ChqError{CHQ_ERR_OUT_OF_MEMORY, "host allocation failed"};
  return p;
}
void HostPool::free(void* p, size_t cap) {
  if (!p) return;
  if (cap >= ((size_t)1 << 20)) {
    std::lock_guard<std::mutex> lk(mu_);
    if (cached_ + cap <= limit_) { free_[cap].push_back(p); cached_ += cap; return; }
  }
  ::free(p);
}
void HostPool::trim() {
  std::unordered_map<size_t, std::vector<void*>> f;
  { std::lock_guard<std::mutex> lk(mu_); f.swap(free_); cached_ = 0; }
  for (auto& kv : f) for (void* p : kv.second) ::free(p);
}
void HostPool::set_limit(size_t bytes) {
  { std::lock_guard<std::mutex> lk(mu_); limit_ = bytes; }
  if (bytes == 0) trim();
}

Buffer::~Buffer() {
  if (!ptr) return;
  // A block released while an exception unwinds the call may still be the source or target of work queued on the context's
  // streams (staged uploads ahead of a typing error, copies behind a kernel that reported a data error): the pools are
  // process-wide, and another context -- another stream -- would get it next.  The fuzz met exactly that: a call's first
  // output columns overwritten by the late upload of an earlier, failed call.  Errors are the slow path: wait for the device.
  if (std::uncaught_exceptions() > 0) (void)hipDeviceSynchronize();
  if (device) DevicePool::instance().free(ptr, cap, device_id); else HostPool::instance().free(ptr, cap);
}
BufferPtr make_device_buffer(size_t bytes, int device) {
  auto b = std::make_shared<Buffer>();
  b->ptr = DevicePool::instance().alloc(bytes ? bytes : 1, device, &b->cap);
  b->bytes = bytes; b->device = true; b->device_id = device;
  return b;
}
BufferPtr make_host_buffer(size_t bytes) {
  auto b = std::make_shared<Buffer>();
  b->ptr = HostPool::instance().alloc(bytes ? bytes : 1, &b->cap);
  b->bytes = bytes; b->device = false;
  return b;
}

// The auxiliary streams and their fork / join events: created together, on the context's device, the first time a call
// needs them (the ONE creation site; `aux_ready` is set only when every object exists, so a failure half way is retried
// from the first missing object instead of leaving null streams behind a non-null event).
void ensure_aux_streams(Context& ctx) {
  if (ctx.aux_ready) return;
  int current = ctx.device;
  (void)hipGetDevice(&current);
  if (current != ctx.device) check_hip(hipSetDevice(ctx.device), "hipSetDevice");
  if (!ctx.aux_fork) check_hip(hipEventCreateWithFlags(&ctx.aux_fork, hipEventDisableTiming), "hipEventCreate");
  for (int i = 0; i < Context::kAuxStreams; ++i) {
    if (!ctx.aux[i]) check_hip(hipStreamCreateWithFlags(&ctx.aux[i], hipStreamNonBlocking), "hipStreamCreate");
    if (!ctx.aux_join[i]) check_hip(hipEventCreateWithFlags(&ctx.aux_join[i], hipEventDisableTiming), "hipEventCreate");
  }
  ctx.aux_ready = true;
}
// Work on the auxiliary streams starts behind everything queued on ctx.stream ...
void fork_aux_streams(Context& ctx) {
  ensure_aux_streams(ctx);
  check_hip(hipEventRecord(ctx.aux_fork, ctx.stream), "hipEventRecord(fork)");
  for (int i = 0; i < Context::kAuxStreams; ++i) check_hip(hipStreamWaitEvent(ctx.aux[i], ctx.aux_fork, 0), "hipStreamWaitEvent(fork)");
}
// ... and ctx.stream goes on only behind everything queued on them (no host synchronisation on either end)
void join_aux_streams(Context& ctx) {
  for (int i = 0; i < Context::kAuxStreams; ++i) {
    check_hip(hipEventRecord(ctx.aux_join[i], ctx.aux[i]), "hipEventRecord(join)");
    check_hip(hipStreamWaitEvent(ctx.stream, ctx.aux_join[i], 0), "hipStreamWaitEvent(join)");
  }
}

void kernel_span_begin(Context& ctx) {
  if (ctx.opt_time_kernels && !ctx.ev0) { check_hip(hipEventCreate(&ctx.ev0), "hipEventCreate"); check_hip(hipEventCreate(&ctx.ev1), "hipEventCreate"); }
  if (ctx.opt_time_kernels) check_hip(hipEventRecord(ctx.ev0, ctx.stream), "hipEventRecord");
}
void kernel_span_end(Context& ctx) { if (ctx.opt_time_kernels) check_hip(hipEventRecord(ctx.ev1, ctx.stream), "hipEventRecord"); }
int64_t kernel_span_ns(Context& ctx) {
  float ms = 0;
  if (ctx.opt_time_kernels) check_hip(hipEventElapsedTime(&ms, ctx.ev0, ctx.ev1), "hipEventElapsedTime");
  return (int64_t)(ms * 1e6);
}

Context::~Context() {
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  if (aux_fork) (void)hipEventDestroy(aux_fork);
  for (hipEvent_t e : upload_events) (void)hipEventDestroy(e);
  for (int i = 0; i < kAuxStreams; ++i) { if (aux_join[i]) (void)hipEventDestroy(aux_join[i]); if (aux[i]) (void)hipStreamDestroy(aux[i]); }
  if (own_stream && stream) (void)hipStreamDestroy(stream);
}

// =================================================================================================
// host worker pool, phase timer
// =================================================================================================
namespace {
class WorkPool {
 public:
  WorkPool() {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned n = std::min(16u, hw) - 1;   // + the calling thread
    for (unsigned i = 0; i < n; ++i) threads_.emplace_back([this] { worker(); });
  }
  ~WorkPool() {
    { std::lock_guard<std::mutex> l(m_); stop_ = true; }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
  }
  unsigned width() const { return (unsigned)threads_.size() + 1; }
  void run(unsigned tasks, const std::function<void(unsigned)>& f) {
    if (tasks == 0) return;
    std::unique_lock<std::mutex> busy(run_m_, std::try_to_lock);
    if (tasks == 1 || threads_.empty() || !busy.owns_lock()) { for (unsigned t = 0; t < tasks; ++t) f(t); return; }
    std::unique_lock<std::mutex> l(m_);
    job_ = &f; next_ = 0; total_ = tasks; finished_ = 0; error_ = nullptr; ++epoch_;
    cv_.notify_all();
    drain(l);
    done_cv_.wait(l, [this] { return finished_ == total_; });
    job_ = nullptr;
    if (error_) { auto e = error_; error_ = nullptr; l.unlock(); std::rethrow_exception(e); }
  }

 private:
  void drain(std::unique_lock<std::mutex>& l) {   // called with m_ held
    while (job_ && next_ < total_) {
      const unsigned t = next_++;
      const auto* f = job_;
      l.unlock();
      std::exception_ptr err;
      try { (*f)(t); } catch (...) { err = std::current_exception(); }
      l.lock();
      if (err && !error_) error_ = err;
      if (++finished_ == total_) done_cv_.notify_all();
    }
  }
  void worker() {
    std::unique_lock<std::mutex> l(m_);
    unsigned seen = 0;
    while (true) {
      cv_.wait(l, [&] { return stop_ || epoch_ != seen; });
      if (stop_) return;
      seen = epoch_;
      drain(l);
    }
  }
  std::vector<std::thread> threads_;
  std::mutex m_, run_m_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(unsigned)>* job_ = nullptr;
  unsigned next_ = 0, total_ = 0, finished_ = 0, epoch_ = 0;
  std::exception_ptr error_;
  bool stop_ = false;
};
WorkPool& work_pool() { static WorkPool p; return p; }
}  // namespace

void pool_run(unsigned tasks, const std::function<void(unsigned)>& f) { work_pool().run(tasks, f); }
unsigned pool_width() { return work_pool().width(); }
void pool_ranges(size_t n, size_t grain, const std::function<void(size_t, size_t)>& f) {
  if (n == 0) return;
  const size_t want = grain ? (n + grain - 1) / grain : 1;
  const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(want, pool_width()));
  const size_t per = (n + T - 1) / T;
  pool_run(T, [&](unsigned t) { const size_t i0 = std::min(n, (size_t)t * per), i1 = std::min(n, (size_t)(t + 1) * per); if (i0 < i1) f(i0, i1); });
}

PhaseTimer::PhaseTimer(const char* w) : what(w) {
  static const bool enabled = [] { const char* e = getenv("CHQ_TIMING"); return e && *e == '1'; }();
  on = enabled;
  if (on) t0 = last = std::chrono::steady_clock::now();
}
void PhaseTimer::mark(const char* phase) {
  if (!on) return;
  const auto now = std::chrono::steady_clock::now();
  line += std::string(" ") + phase + "=" + std::to_string(std::chrono::duration<double, std::micro>(now - last).count()).substr(0, 8) + "us";
  last = now;
}
PhaseTimer::~PhaseTimer() {
  if (!on) return;
  fprintf(stderr, "[chq timing] %s total=%.1fus%s\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), line.c_str());
}

}  // namespace chq
