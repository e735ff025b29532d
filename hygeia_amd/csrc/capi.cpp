// capi.cpp -- the C ABI of include/hygeia_amd.h: model construction (host
// tables, upload), workspace planning, chain descriptors, launches. Compiled by
// hipcc into hygeia_amd/lib/libhygeia_amd.so together with tg_kernels.hip.
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hyg_arith.h"
#include "../../include/hygeia_amd.h"
#include "../../include/hyg_sg_model.h"
#include "sg_common.h"
#include "tg_common.h"
#include "dmp_common.h"
#include "dmr_common.h"
#include "cp_common.h"
#include "em_common.h"

namespace hyg {
int bed_launch_labels(const double* probs, int K, int64_t n, int8_t* label, double* score, void* stream);
int pre_launch_collapse(const int64_t* pos0, int64_t T, const int64_t* plus_start, const int64_t* plus_end,
                        const double* plus_cov, const double* plus_pct, int64_t n_plus, const int64_t* minus_start,
                        const double* minus_cov, const double* minus_pct, int64_t n_minus, int single_base,
                        uint8_t* matched, double* out, int stride, int col, int* conflicts, void* stream);
}

using namespace hyg;

namespace {

thread_local std::string g_err;

// the process's device slot (hyg_device_slot_acquire): the descriptor holding the flock
std::mutex g_slot_mu;
int g_slot_fd = -1, g_slot_device = -1, g_slot_index = -1;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

bool have_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return n > 0;
}

template <typename T>
hipError_t dmalloc_copy(T** dst, const T* src, size_t count) {
  hipError_t e = hipMalloc((void**)dst, sizeof(T) * (count ? count : 1));
  if (e != hipSuccess) return e;
  if (count) e = hipMemcpy(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice);
  return e;
}

// The current HIP device must be the one a model's tables live on.
bool on_model_device(int device) {
  int cur = -1;
  return hipGetDevice(&cur) == hipSuccess && cur == device;
}

// Every model of a launch (hyg_tg_model or hyg_sg_model) must have its tables
// on a device, and on the current one. Checked before anything is allocated.
template <typename M>
int models_on_device(const M* const* models, int32_t n_models) {
  for (int k = 0; k < n_models; ++k) {
    if (!models[k]->on_device) return fail(HYG_EDEVICE, "no HIP device: hygeia_amd has no CPU fallback");
    if (!on_model_device(models[k]->device))
      return fail(HYG_EINVAL, "the current HIP device is not the model's device");
  }
  return HYG_OK;
}

// RAII device allocation with the blocking copies of the host forms. Size 0
// allocates a byte and copies nothing; a null host pointer (an optional array
// the caller left out) is skipped.
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  bool alloc(size_t n) { return hipMalloc(&p, n ? n : 1) == hipSuccess; }
  bool alloc_for(const void* host, size_t n) { return !host || alloc(n); }  // an optional array: only when given
  bool upload(const void* host, size_t n) const {
    return !host || n == 0 || hipMemcpy(p, host, n, hipMemcpyHostToDevice) == hipSuccess;
  }
  bool download(void* host, size_t n) const {
    return !host || n == 0 || hipMemcpy(host, p, n, hipMemcpyDeviceToHost) == hipSuccess;
  }
};

// The stream-ordered buffer of a launch's estimation inputs: freed on the
// stream, behind the kernels that read it, when the launching call returns.
struct AsyncBuf {
  void* p = nullptr;
  hipStream_t s = nullptr;
  ~AsyncBuf() {
    if (p) (void)hipFreeAsync(p, s);
  }
  bool alloc(size_t n, hipStream_t stream) {
    s = stream;
    return hipMallocAsync(&p, n, s) == hipSuccess;
  }
};

// The tail of every chain launch: the launcher's code as the entry's.
int launch_result(int rc, const std::string& unsupported) {
  if (rc == HYG_EUNSUPPORTED) return fail(rc, unsupported);
  if (rc != HYG_OK) return fail(rc, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
  return HYG_OK;
}

int32_t copy_name(const char* name, char* buf, int32_t len) {
  const int32_t need = (int32_t)std::strlen(name) + 1;
  if (buf && len > 0) std::snprintf(buf, (size_t)len, "%s", name);
  return need;
}

// Host-to-device upload of per-launch descriptors through a pinned buffer owned
// by the model: the async copy reads memory that outlives the call, and the
// buffer is reused only once the previous upload from it has completed.
struct PinnedStage {
  void* p = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool pending = false;

  hipError_t upload(void* dst, const void* src, size_t n, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (pending) {
      e = hipEventSynchronize(ev);
      if (e != hipSuccess) return e;
      pending = false;
    }
    if (!ev && (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
    if (n > cap) {
      if (p) (void)hipHostFree(p);
      p = nullptr;
      cap = 0;
      if ((e = hipHostMalloc(&p, n, hipHostMallocDefault)) != hipSuccess) return e;
      cap = n;
    }
    std::memcpy(p, src, n);
    if ((e = hipMemcpyAsync(dst, p, n, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    if ((e = hipEventRecord(ev, s)) != hipSuccess) return e;
    pending = true;
    return hipSuccess;
  }
  void release() {
    if (pending) (void)hipEventSynchronize(ev);
    if (ev) (void)hipEventDestroy(ev);
    if (p) (void)hipHostFree(p);
    p = nullptr;
    ev = nullptr;
    cap = 0;
    pending = false;
  }
};

// One pinned stage per stream, each behind its own mutex: host threads that
// share a model on different streams neither race on a buffer nor wait for
// each other's kernels (an upload waits only for the previous upload of its
// own stream); two threads on one stream take turns.
class PinnedStages {
 public:
  hipError_t upload(void* dst, const void* src, size_t n, hipStream_t s) {
    Slot* slot;
    {
      std::lock_guard<std::mutex> g(mu_);
      std::unique_ptr<Slot>& u = by_stream_[s];
      if (!u) u.reset(new Slot);
      slot = u.get();
    }
    std::lock_guard<std::mutex> g(slot->mu);
    return slot->st.upload(dst, src, n, s);
  }
  void release() {
    std::lock_guard<std::mutex> g(mu_);
    for (auto& kv : by_stream_) {
      std::lock_guard<std::mutex> gs(kv.second->mu);
      kv.second->st.release();
    }
    by_stream_.clear();
  }

 private:
  struct Slot {
    std::mutex mu;
    PinnedStage st;
  };
  std::mutex mu_;
  std::map<hipStream_t, std::unique_ptr<Slot>> by_stream_;
};

}  // namespace

struct hyg_tg_model {
  hyg_tg_consts c{};
  int32_t dcap = 0;
  int32_t nmax_reads = 0;
  int32_t max_duration = 0;
  double mu[HYG_KMAX] = {}, sigma[HYG_KMAX] = {};  // as given (hyg_tg_models_compatible compares their bits)
  std::vector<double> hz, lf, lg, cst, bbt;
  bool on_device = false;
  int device = -1;
  hyg_tg_consts* d_consts = nullptr;
  double* d_hz = nullptr;
  double* d_lf = nullptr;
  double* d_lg = nullptr;
  double* d_cst = nullptr;
  double* d_bbt = nullptr;
  mutable PinnedStages stage;  // descriptor uploads (thread-safe, one pinned buffer per stream)

  ModelDev dev() const {
    ModelDev m{};
    m.consts = d_consts;
    m.hz = d_hz;
    m.dcap = dcap;
    m.nmax_reads = nmax_reads;
    m.lf = d_lf;
    m.lg = d_lg;
    m.cst = d_cst;
    m.bbt = d_bbt;
    return m;
  }
};

// The emission's per-(n, y) term table is built when it stays L2-sized (the
// pipeline's coverage: max reads ~170, 0.7 MB at K = 6); beyond that the
// emission forms each term from the lgamma rows.
constexpr size_t kBbtMaxBytes = (size_t)16 << 20;

struct hyg_sg_model {
  hyg_sg_consts c{};
  hyg_sg_params params{};  // as given (initial theta, kappa) for the estimation path
  int32_t dcap = 0;
  int32_t nmax_reads = 0;
  int32_t max_duration = 0;
  std::vector<double> hz, lf, lg, cst;
  std::vector<uint8_t> ex;
  bool on_device = false;
  int device = -1;
  mutable PinnedStages stage;  // descriptor uploads (thread-safe, one pinned buffer per stream)
  hyg_sg_consts* d_consts = nullptr;
  double* d_hz = nullptr;
  uint8_t* d_ex = nullptr;
  double* d_lf = nullptr;
  double* d_lg = nullptr;
  double* d_cst = nullptr;

  SgModelDev dev() const {
    SgModelDev m{};
    m.consts = d_consts;
    m.hz = d_hz;
    m.ex = d_ex;
    m.dcap = dcap;
    m.nmax_reads = nmax_reads;
    m.lf = d_lf;
    m.lg = d_lg;
    m.cst = d_cst;
    return m;
  }
};

extern "C" {

const char* hyg_version(void) { return "hygeia_amd 0.1.0 (gfx950)"; }

const char* hyg_last_error(void) { return g_err.c_str(); }

int hyg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int hyg_device_slot_acquire(const char* lock_dir, int32_t n_devices, int32_t max_per_device, int32_t* device,
                            int32_t* slot) {
  if (!lock_dir || !device || !slot) return fail(HYG_EINVAL, "null argument");
  if (n_devices < 1 || max_per_device < 1) return fail(HYG_EINVAL, "n_devices and max_per_device must be >= 1");
  std::lock_guard<std::mutex> g(g_slot_mu);
  if (g_slot_fd >= 0) {  // one slot per process
    *device = g_slot_device;
    *slot = g_slot_index;
    return HYG_OK;
  }
  for (int j = 0; j < max_per_device; ++j) {
    for (int d = 0; d < n_devices; ++d) {
      const std::string path =
          std::string(lock_dir) + "/hygeia_amd.gpu" + std::to_string(d) + ".slot" + std::to_string(j) + ".lock";
      int fd = ::open(path.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0666);
      if (fd < 0 && errno == EACCES) fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);  // another user's file
      if (fd < 0) return fail(HYG_EINVAL, "device slot lock " + path + ": " + std::strerror(errno));
      if (::flock(fd, LOCK_EX | LOCK_NB) == 0) {
        g_slot_fd = fd;
        g_slot_device = d;
        g_slot_index = j;
        *device = d;
        *slot = j;
        return HYG_OK;
      }
      const int err = errno;
      ::close(fd);
      if (err != EWOULDBLOCK) return fail(HYG_EINVAL, "device slot lock " + path + ": " + std::strerror(err));
    }
  }
  return fail(HYG_EINVAL, "every device slot is held");
}

int hyg_device_slot_release(void) {
  std::lock_guard<std::mutex> g(g_slot_mu);
  if (g_slot_fd >= 0) ::close(g_slot_fd);  // closing the only descriptor drops the flock
  g_slot_fd = -1;
  g_slot_device = g_slot_index = -1;
  return HYG_OK;
}

int hyg_set_device(int32_t device) {
  const int n = hyg_device_count();
  if (n < 1) return fail(HYG_EDEVICE, "no HIP device");
  if (device < 0 || device >= n) return fail(HYG_EINVAL, "device out of range");
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail(HYG_EDEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
  return HYG_OK;
}

int hyg_get_device(void) {
  int d = -1;
  if (hipGetDevice(&d) != hipSuccess) {
    (void)hipGetLastError();
    return fail(HYG_EDEVICE, "no HIP device");
  }
  return d;
}

void hyg_tg_params_default(hyg_tg_params* p) {
  std::memset(p, 0, sizeof(*p));
  const double mu[6] = {0.95, 0.05, 0.80, 0.20, 0.50, 0.50};
  const double sg[6] = {0.05, 0.05, 0.1, 0.1, 0.1, 0.2886751};
  p->n_regimes = 6;
  p->minimum_duration = 3;
  p->num_resampled_ancestors = 50;
  p->num_samples_backward = 25;
  p->optimal_resampling = 1;
  p->multinomial = 0;
  for (int i = 0; i < 6; ++i) {
    p->mu[i] = mu[i];
    p->sigma[i] = sg[i];
  }
  // uniform off-diagonal transitions, omega = 0.8
  p->theta_len = 36;
  for (int i = 0; i < 30; ++i) p->theta[i] = 0.0;
  for (int i = 30; i < 36; ++i) p->theta[i] = std::log(0.8 / 0.2);
  p->omega_case = 0.8;
  p->merge_log_prob = std::log(0.1);
  p->split_prob = 0.01;
  p->kappa_control = 2.0;
  p->kappa_case = 2.0;
}

void hyg_tg_model_destroy(hyg_tg_model* m) {
  if (!m) return;
  if (m->on_device) {
    m->stage.release();
    (void)hipFree(m->d_consts);
    (void)hipFree(m->d_hz);
    (void)hipFree(m->d_lf);
    (void)hipFree(m->d_lg);
    (void)hipFree(m->d_cst);
    (void)hipFree(m->d_bbt);
  }
  delete m;
}

int hyg_tg_model_create(const hyg_tg_params* params, int32_t max_total_reads, int32_t max_duration,
                        hyg_tg_model** out) {
  if (!params || !out) return fail(HYG_EINVAL, "null argument");
  *out = nullptr;
  if (max_total_reads < 0 || max_total_reads > 65535) return fail(HYG_EINVAL, "max_total_reads out of [0, 65535]");
  if (max_duration < 1 || max_duration >= HYG_DMAX - 2) return fail(HYG_EINVAL, "max_duration out of range");
  auto* m = new hyg_tg_model();
  int rc = hyg_tg_derive(params, &m->c);
  if (rc != HYG_OK) {
    delete m;
    return fail(rc, "invalid model parameters");
  }
  m->max_duration = max_duration;
  m->nmax_reads = max_total_reads;
  std::memcpy(m->mu, params->mu, sizeof(double) * m->c.K);
  std::memcpy(m->sigma, params->sigma, sizeof(double) * m->c.K);
  m->dcap = hyg_hazard_len(&m->c, max_duration + 2);
  const int K = m->c.K, L = max_total_reads + 1;
  m->hz.resize((size_t)2 * K * m->dcap * 2);
  hyg_hazard_fill(&m->c, m->dcap, m->hz.data());
  m->lf.resize(L);
  m->lg.resize((size_t)3 * K * L);
  m->cst.resize(K);
  hyg_bb_tables(&m->c, max_total_reads, m->lf.data(), m->lg.data(), m->cst.data());
  if (hyg_bb_term_table_len(K, max_total_reads) * sizeof(double) <= kBbtMaxBytes) {
    m->bbt.resize(hyg_bb_term_table_len(K, max_total_reads));
    hyg_bb_term_table(K, max_total_reads, m->lf.data(), m->lg.data(), m->cst.data(), m->bbt.data());
  }
  if (have_device()) {
    (void)hipGetDevice(&m->device);
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = dmalloc_copy(&m->d_consts, &m->c, 1);
    if (e == hipSuccess) e = dmalloc_copy(&m->d_hz, m->hz.data(), m->hz.size());
    if (e == hipSuccess) e = dmalloc_copy(&m->d_lf, m->lf.data(), m->lf.size());
    if (e == hipSuccess) e = dmalloc_copy(&m->d_lg, m->lg.data(), m->lg.size());
    if (e == hipSuccess) e = dmalloc_copy(&m->d_cst, m->cst.data(), m->cst.size());
    if (e == hipSuccess && !m->bbt.empty()) e = dmalloc_copy(&m->d_bbt, m->bbt.data(), m->bbt.size());
    m->on_device = true;
    if (e != hipSuccess) {
      hyg_tg_model_destroy(m);
      return fail(HYG_EDEVICE, std::string("device upload failed: ") + hipGetErrorString(e));
    }
  }
  *out = m;
  return HYG_OK;
}

int32_t hyg_tg_num_particles(const hyg_tg_model* m) { return m ? m->c.Nmax : 0; }

int32_t hyg_tg_global_weights(const hyg_tg_model* m) { return (m && hyg::forward_global_w(m->c)) ? 1 : 0; }

int32_t hyg_tg_threads_per_chain(const hyg_tg_model* m, int32_t n_chains) {
  return m ? hyg::tg_threads_per_chain(m->c, n_chains) : 0;
}

int32_t hyg_tg_backward_threads_per_chain(const hyg_tg_model* m, int32_t n_chains) {
  return m ? hyg::tg_threads_per_chain_bwd(m->c, n_chains) : 0;
}

int32_t hyg_tg_chains_per_cu(const hyg_tg_model* m, int32_t n_chains) {
  if (!m || !m->on_device) return 0;
  return hyg::tg_resident_per_cu(m->c, n_chains);
}

size_t hyg_tg_lds_bytes(const hyg_tg_model* m, int32_t threads, int32_t backward) {
  return m ? hyg::tg_layout_bytes(m->c, threads, backward != 0) : 0;
}

}  // extern "C"

// ------------------------------------- two-group host launch layer
// One set of helpers under all of hyg_tg_{run,filter,trace}_chains[_host][_multi]
// and the kernel-name entries ("Host launch layer"): a new launch
// family adds a TgKind and an output set, not a copy of these.
namespace {

// The refusal of a shape no chain kernel runs (the plan's HYG_EUNSUPPORTED).
std::string unsupported_shape(const hyg_tg_model* m) {
  if (m->c.M > 256)
    return "num_resampled_particles M = " + std::to_string(m->c.M) +
           " exceeds 256 (one resampled ancestor per thread of a 256-thread workgroup)";
  return "the chain kernels' LDS layout exceeds the 160 KiB of a CU at every workgroup size";
}
int fail_unsupported_shape(const hyg_tg_model* m) { return fail(HYG_EUNSUPPORTED, unsupported_shape(m)); }

size_t header_bytes(int32_t n_chains) {
  const size_t h = sizeof(ChainDev) * (size_t)n_chains + (sizeof(int32_t) + sizeof(double)) * (size_t)n_chains;
  return (h + 255) / 256 * 256;
}

// The model table of a multi-model launch stands behind the chain descriptors
// in the workspace header (one upload carries both); the default status and the
// log Z area follow it.
size_t header_bytes_multi(int32_t n_chains, int32_t n_models) {
  return (header_bytes(n_chains) + sizeof(ModelDev) * (size_t)n_models + 255) / 256 * 256;
}

// The scratch of a chain in a forward-only launch: that of a shape whose
// forward keeps its particle arrays in global memory, and none that only the
// backward uses (the C5 shape's).
size_t filter_scratch_bytes(const hyg_tg_consts& c) { return forward_global_w(c) ? chain_scratch_bytes(c) : 0; }

// Whether models can share a launch (hyg_tg_models_compatible): the message
// names the first field that differs.
int models_compatible(const hyg_tg_model* const* models, int32_t n_models) {
  if (!models || n_models < 1) return fail(HYG_EINVAL, "no models");
  for (int i = 0; i < n_models; ++i)
    if (!models[i]) return fail(HYG_EINVAL, "null model " + std::to_string(i));
  const hyg_tg_model* a = models[0];
  for (int i = 1; i < n_models; ++i) {
    const hyg_tg_model* b = models[i];
    const char* field = nullptr;
    if (a->c.K != b->c.K) field = "n_regimes";
    else if (a->c.u != b->c.u) field = "minimum_duration";
    else if (a->c.M != b->c.M) field = "num_resampled_ancestors";
    else if (a->c.B != b->c.B) field = "num_samples_backward";
    else if (a->c.optimal != b->c.optimal) field = "optimal_resampling";
    else if (a->nmax_reads != b->nmax_reads) field = "max_total_reads";
    else if (std::memcmp(a->mu, b->mu, sizeof(double) * a->c.K) != 0) field = "mu";
    else if (std::memcmp(a->sigma, b->sigma, sizeof(double) * a->c.K) != 0) field = "sigma";
    if (field)
      return fail(HYG_EINVAL, std::string("models 0 and ") + std::to_string(i) + " differ in " + field +
                                  ": the models of one launch share the shape and the emission table");
  }
  return HYG_OK;
}

// (both families)
int check_chain_models(const int32_t* chain_model, int32_t n_chains, int32_t n_models) {
  if (!chain_model) return fail(HYG_EINVAL, "null chain_model");
  for (int i = 0; i < n_chains; ++i)
    if (chain_model[i] < 0 || chain_model[i] >= n_models)
      return fail(HYG_EINVAL, "chain_model[" + std::to_string(i) + "] = " + std::to_string(chain_model[i]) +
                                  " out of [0, " + std::to_string(n_models) + ")");
  return HYG_OK;
}

// The read counts of the host forms: meth <= tot <= the model's max_total_reads.
int tg_check_counts(const hyg_tg_model* m, const uint16_t* meth_c, const uint16_t* tot_c, int64_t n_c,
                    const uint16_t* meth_k, const uint16_t* tot_k, int64_t n_k) {
  for (int64_t i = 0; i < n_c; ++i)
    if (meth_c[i] > tot_c[i] || tot_c[i] > m->nmax_reads) return fail(HYG_EINVAL, "invalid control counts");
  for (int64_t i = 0; i < n_k; ++i)
    if (meth_k[i] > tot_k[i] || tot_k[i] > m->nmax_reads) return fail(HYG_EINVAL, "invalid case counts");
  return HYG_OK;
}

// The kernel-name entries: the forward or the backward of a smoothing launch,
// the forward-only kernel, the traced one.
enum TgName { kNameForward, kNameBackward, kNameFilter, kNameTrace };
int32_t tg_name_impl(const hyg_tg_model* const* models, int32_t n_models, bool multi, TgName which, int32_t n_chains,
                     char* buf, int32_t len) {
  if (len < 0) return fail(HYG_EINVAL, "negative length");
  const int rc = models_compatible(models, n_models);
  if (rc != HYG_OK) return rc;
  const hyg_tg_consts& c = models[0]->c;
  const char* name = nullptr;
  const int st = which == kNameFilter  ? hyg::tg_filter_kernel_name(c, n_chains, &name, multi)
                 : which == kNameTrace ? hyg::tg_trace_kernel_name(c, n_chains, &name, multi)
                                       : hyg::tg_kernel_name(c, n_chains, which == kNameBackward, &name, multi);
  if (st != HYG_OK) return fail_unsupported_shape(models[0]);
  return copy_name(name, buf, len);
}

// The kinds of chain launch: forward, history and backward simulation; the
// forward alone (log Z); the forward alone with a per-site trace.
enum TgKind { kSmooth, kFilter, kTrace };

bool trace_empty(const hyg_tg_trace* t) { return !t || (!t->log_z_t && !t->split_probs && !t->regime_probs); }
const char kNoTrace[] = "no trace array (hyg_tg_filter_chains is the launch without one)";

// Validates the chains of a launch and builds its upload image: ChainDev
// [n_chains] and, for a multi-model launch (chain_model non-null), the model
// table behind them. Lays out the workspace -- header | the chains' records |
// to a multiple of 256 | the chains' scratch -- and returns its size in *need.
// A forward-only launch is that layout with a record size of 0 (ws_offset 0)
// and the forward's scratch alone; its out_begin counts only when traced.
int tg_fill_upload(const hyg_tg_model* const* models, int32_t n_models, const int32_t* chain_model,
                   const hyg_tg_chain* chains, int32_t n_chains, TgKind kind, std::vector<uint8_t>& up, size_t* need) {
  const hyg_tg_model* m = models[0];
  const bool multi = chain_model != nullptr;
  const size_t cd_bytes = sizeof(ChainDev) * (size_t)n_chains;
  up.assign(cd_bytes + (multi ? sizeof(ModelDev) * (size_t)n_models : 0), 0);
  ChainDev* cd = (ChainDev*)up.data();
  const size_t rb = kind == kSmooth ? record_bytes(m->c.M) : 0;
  const size_t sb = kind == kSmooth ? chain_scratch_bytes(m->c) : filter_scratch_bytes(m->c);
  const bool rows = kind != kFilter;
  size_t off = multi ? header_bytes_multi(n_chains, n_models) : header_bytes(n_chains);
  for (int i = 0; i < n_chains; ++i) {
    const hyg_tg_chain& c = chains[i];
    if (c.n_sites < 1) return fail(HYG_EINVAL, "chain with no sites");
    if (c.n_sites > models[multi ? chain_model[i] : 0]->max_duration)
      return fail(HYG_EINVAL, "chain longer than the model's max_duration");
    if (c.site_begin < 0 || (rows && c.out_begin < 0)) return fail(HYG_EINVAL, "negative chain offset");
    cd[i].site_begin = c.site_begin;
    cd[i].out_begin = rows ? c.out_begin : 0;
    cd[i].ws_offset = rb ? (int64_t)off : 0;
    cd[i].seed = c.seed;
    cd[i].chain_id = c.chain_id;
    cd[i].T = c.n_sites;
    cd[i].pad = multi ? chain_model[i] : 0;
    off += (size_t)c.n_sites * rb;
  }
  // the global particle scratch of each chain, behind the records
  off = (off + 255) / 256 * 256;
  for (int i = 0; i < n_chains; ++i) {
    cd[i].wg_offset = sb ? (int64_t)off : 0;
    off += sb;
  }
  for (int k = 0; multi && k < n_models; ++k) {
    const ModelDev md = models[k]->dev();
    std::memcpy(up.data() + cd_bytes + sizeof(ModelDev) * (size_t)k, &md, sizeof(ModelDev));
  }
  *need = off;
  return HYG_OK;
}

// The device forms behind their entries' own first checks, and the launch of
// the host forms. chain_model == nullptr: the one model models[0]; else chain i
// runs with models[chain_model[i]] (models_compatible and check_chain_models
// have passed). out: a forward-only kind reads log_z, final_log_weights and
// status alone; trace: the device arrays of kTrace.
int tg_launch(const hyg_tg_model* const* models, int32_t n_models, const int32_t* chain_model,
              const hyg_tg_chain* chains, int32_t n_chains, const double* E, void* workspace, size_t workspace_bytes,
              TgKind kind, const hyg_tg_outputs* out, const hyg_tg_trace* trace, void* stream) {
  const hyg_tg_model* m = models[0];
  const bool multi = chain_model != nullptr, smooth = kind == kSmooth;
  if (!chains || !out || !E || !workspace) return fail(HYG_EINVAL, "null argument");
  if (int rc = models_on_device(models, n_models)) return rc;
  if (n_chains <= 0) return HYG_OK;
  if (!out->log_z ||
      (smooth && (!out->merged || !out->control || !out->kase || !out->split_probs || !out->regime_probs)))
    return fail(HYG_EINVAL, "null output buffer");
  if (!m->c.optimal) return fail(HYG_EUNSUPPORTED, "optimal_resampling = 0 is not implemented on the GPU path");
  std::vector<uint8_t> up;
  size_t need = 0;
  if (int rc = tg_fill_upload(models, n_models, chain_model, chains, n_chains, kind, up, &need)) return rc;
  if (need > workspace_bytes)
    return fail(HYG_EINVAL, std::string("workspace too small (see ") +
                                (smooth ? "hyg_tg_workspace_bytes" : "hyg_tg_filter_workspace_bytes") +
                                (multi ? "_multi)" : ")"));
  uint8_t* ws = (uint8_t*)workspace;
  if (m->stage.upload(ws, up.data(), up.size(), (hipStream_t)stream) != hipSuccess)
    return fail(HYG_EDEVICE, "descriptor upload failed");
  hyg_tg_outputs o = *out;
  if (!o.status) o.status = (int32_t*)(ws + up.size());  // the default status area, behind the upload
  const ChainDev* cd = (const ChainDev*)ws;              // on the device; up.data(): the same on the host
  const ModelDev* table = (const ModelDev*)(ws + sizeof(ChainDev) * (size_t)n_chains);
  int rc;
  if (smooth)
    rc = multi ? launch_chains_multi(table, m->c, cd, n_chains, E, ws, o, stream, (const ChainDev*)up.data())
               : launch_chains(m->dev(), m->c, cd, n_chains, E, ws, o, stream, (const ChainDev*)up.data());
  else if (kind == kTrace)
    rc = multi ? launch_trace_multi(table, m->c, cd, n_chains, E, ws, o, *trace, stream)
               : launch_trace(m->dev(), m->c, cd, n_chains, E, ws, o, *trace, stream);
  else
    rc = multi ? launch_filter_multi(table, m->c, cd, n_chains, E, ws, o, stream)
               : launch_filter(m->dev(), m->c, cd, n_chains, E, ws, o, stream);
  return launch_result(rc, unsupported_shape(m));
}

// The six device entries: what each refuses before tg_launch's null-argument
// and device checks. A single-model entry has refused a null model. The traced
// entries check the trace and the workspace here, before the device.
int tg_launch_entry(const hyg_tg_model* const* models, int32_t n_models, bool multi, const int32_t* chain_model,
                    const hyg_tg_chain* chains, int32_t n_chains, const double* E, void* workspace,
                    size_t workspace_bytes, TgKind kind, const hyg_tg_outputs* out, const hyg_tg_trace* trace,
                    void* stream) {
  int rc;
  if (multi && (rc = models_compatible(models, n_models)) != HYG_OK) return rc;
  if (kind == kTrace && trace_empty(trace)) return fail(HYG_EINVAL, kNoTrace);
  if (multi && n_chains > 0 && (rc = check_chain_models(chain_model, n_chains, n_models)) != HYG_OK) return rc;
  if (!multi || n_chains <= 0) chain_model = nullptr;  // (nothing to run: the single-model checks of the arguments)
  if (kind == kTrace && n_chains > 0 &&
      workspace_bytes < (multi ? hyg_tg_filter_workspace_bytes_multi(models, n_models, n_chains)
                               : hyg_tg_filter_workspace_bytes(models[0], n_chains)))
    return fail(HYG_EINVAL, "workspace too small (see hyg_tg_filter_workspace_bytes[_multi])");
  return tg_launch(models, n_models, chain_model, chains, n_chains, E, workspace, workspace_bytes, kind, out, trace,
                   stream);
}

hyg_tg_outputs forward_outputs(double* log_z, double* final_w, int32_t* status) {
  hyg_tg_outputs o{};
  o.log_z = log_z;
  o.final_log_weights = final_w;
  o.status = status;
  return o;
}

// The host arrays of a host form, the output set of its kind: kSmooth all but
// log_z_t; kFilter log_z, final_w (optional) and status; kTrace those and the
// trace arrays log_z_t, split, regime (at least one), which have out_rows rows,
// go to the device as they are and come back with the chains' rows written, so
// rows that no chain owns keep what the caller put there.
struct TgHostOut {
  int16_t *merged, *control, *kase;
  float *split, *regime;
  double *log_z_t, *log_z, *final_w;
  int32_t* status;
  int64_t out_rows;
};

// The six host forms. A single-model entry (multi false, chain_model null) has
// refused a null model.
int tg_launch_host(const hyg_tg_model* const* models, int32_t n_models, bool multi, const int32_t* chain_model,
                   const uint16_t* meth_c, const uint16_t* tot_c, int32_t s_c, const uint16_t* meth_k,
                   const uint16_t* tot_k, int32_t s_k, int64_t n_sites, const hyg_tg_chain* chains, int32_t n_chains,
                   TgKind kind, const TgHostOut& h) {
  const bool smooth = kind == kSmooth, traced = kind == kTrace;
  const int64_t out_rows = h.out_rows;
  int rc;
  if (multi && (rc = models_compatible(models, n_models)) != HYG_OK) return rc;
  if (traced) {  // the checks of the traced entries that need no device, made before anything else
    if (!h.log_z_t && !h.split && !h.regime) return fail(HYG_EINVAL, kNoTrace);
    if (!chains || n_chains < 1) return fail(HYG_EINVAL, "empty or negative size");
    for (int i = 0; i < n_chains; ++i)
      if (chains[i].n_sites < 1 || chains[i].out_begin < 0 || chains[i].out_begin + chains[i].n_sites > out_rows)
        return fail(HYG_EINVAL, "chain outside the output rows");
  }
  if (multi) {
    if (n_chains < 1) return fail(HYG_EINVAL, "empty or negative size");
    if ((rc = check_chain_models(chain_model, n_chains, n_models)) != HYG_OK) return rc;
  }
  const hyg_tg_model* m = models[0];
  if ((rc = models_on_device(models, n_models)) != HYG_OK) return rc;
  if (n_sites < 1 || n_chains < 1 || (smooth && out_rows < 1) || s_c < 0 || s_k < 0)
    return fail(HYG_EINVAL, "empty or negative size");
  if (!chains || !h.log_z || !h.status || (smooth && (!h.merged || !h.control || !h.kase || !h.split || !h.regime)))
    return fail(HYG_EINVAL, "null argument");
  if ((s_c && (!meth_c || !tot_c)) || (s_k && (!meth_k || !tot_k))) return fail(HYG_EINVAL, "null count buffer");
  int64_t steps = 0;
  for (int i = 0; i < n_chains; ++i) {
    const hyg_tg_chain& c = chains[i];
    const bool in_sites = c.n_sites >= 1 && c.site_begin >= 0 && c.site_begin + c.n_sites <= n_sites;
    const bool in_rows = kind == kFilter || (c.out_begin >= 0 && c.out_begin + c.n_sites <= out_rows);
    if (smooth && !(in_sites && in_rows)) return fail(HYG_EINVAL, "chain outside the sites or the output rows");
    if (!in_sites) return fail(HYG_EINVAL, "chain outside the sites");
    if (!in_rows) return fail(HYG_EINVAL, "chain outside the output rows");
    steps += c.n_sites;
  }
  const size_t nc = (size_t)n_sites * s_c, nk = (size_t)n_sites * s_k;
  if ((rc = tg_check_counts(m, meth_c, tot_c, (int64_t)nc, meth_k, tot_k, (int64_t)nk)) != HYG_OK) return rc;
  const size_t K = m->c.K, B = m->c.B, Nmax = m->c.Nmax, nch = (size_t)n_chains;
  const size_t R = kind == kFilter ? 0 : (size_t)out_rows;
  const size_t wsb = smooth ? (multi ? hyg_tg_workspace_bytes_multi(models, n_models, n_chains, steps)
                                     : hyg_tg_workspace_bytes(m, n_chains, steps))
                            : (multi ? hyg_tg_filter_workspace_bytes_multi(models, n_models, n_chains)
                                     : hyg_tg_filter_workspace_bytes(m, n_chains));
  DevBuf b_mc, b_tc, b_mk, b_tk, b_E, b_ws, b_mg, b_ct, b_ks, b_zt, b_sp, b_rp, b_lz, b_fw, b_st;
  const bool ok = b_mc.alloc(nc * 2) && b_tc.alloc(nc * 2) && b_mk.alloc(nk * 2) && b_tk.alloc(nk * 2) &&
                  b_E.alloc(sizeof(double) * (size_t)n_sites * 2 * K) && b_ws.alloc(wsb) &&
                  b_mg.alloc_for(h.merged, 2 * R * B) && b_ct.alloc_for(h.control, 4 * R * B) &&
                  b_ks.alloc_for(h.kase, 4 * R * B) && b_zt.alloc_for(h.log_z_t, 8 * R) &&
                  b_sp.alloc_for(h.split, 4 * R) && b_rp.alloc_for(h.regime, 4 * R * 2 * K) && b_lz.alloc(8 * nch) &&
                  b_fw.alloc_for(h.final_w, 8 * nch * Nmax) && b_st.alloc(4 * nch);
  if (!ok) return fail(HYG_ENOMEM, "device allocation failed");
  if (!b_mc.upload(meth_c, nc * 2) || !b_tc.upload(tot_c, nc * 2) || !b_mk.upload(meth_k, nk * 2) ||
      !b_tk.upload(tot_k, nk * 2))
    return fail(HYG_EDEVICE, "copy failed");
  if (traced && (!b_zt.upload(h.log_z_t, 8 * R) || !b_sp.upload(h.split, 4 * R) || !b_rp.upload(h.regime, 4 * R * 2 * K)))
    return fail(HYG_EDEVICE, "copy failed");
  rc = hyg_tg_emission(m, (uint16_t*)b_mc.p, (uint16_t*)b_tc.p, s_c, (uint16_t*)b_mk.p, (uint16_t*)b_tk.p, s_k,
                       n_sites, (double*)b_E.p, nullptr);
  if (rc) return rc;
  hyg_tg_outputs o = forward_outputs((double*)b_lz.p, (double*)b_fw.p, (int32_t*)b_st.p);
  if (smooth) {
    o.merged = (int16_t*)b_mg.p;
    o.control = (int16_t*)b_ct.p;
    o.kase = (int16_t*)b_ks.p;
    o.split_probs = (float*)b_sp.p;
    o.regime_probs = (float*)b_rp.p;
  }
  const hyg_tg_trace dtrace{(double*)b_zt.p, (float*)b_sp.p, (float*)b_rp.p};
  rc = tg_launch(models, n_models, chain_model, chains, n_chains, (double*)b_E.p, b_ws.p, wsb, kind, &o,
                 traced ? &dtrace : nullptr, nullptr);
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(HYG_EDEVICE, "kernel execution failed");
  if (!b_st.download(h.status, 4 * nch) || !b_mg.download(h.merged, 2 * R * B) ||
      !b_ct.download(h.control, 4 * R * B) || !b_ks.download(h.kase, 4 * R * B) || !b_zt.download(h.log_z_t, 8 * R) ||
      !b_sp.download(h.split, 4 * R) || !b_rp.download(h.regime, 4 * R * 2 * K) || !b_lz.download(h.log_z, 8 * nch) ||
      !b_fw.download(h.final_w, 8 * nch * Nmax))
    return fail(HYG_EDEVICE, "copy failed");
  return HYG_OK;
}

}  // namespace

extern "C" {

int hyg_tg_force_threads(int32_t forward, int32_t backward) {
  const int rc = hyg::tg_force_threads(forward, backward);
  return rc == HYG_OK ? rc : fail(rc, "unsupported workgroup size");
}

int hyg_tg_set_tail_overlap(int32_t on) {
  hyg::tg_set_tail_overlap(on != 0);
  return HYG_OK;
}

int hyg_tg_set_gather_window(int32_t positions) {
  const int rc = hyg::tg_set_gather_window(positions);
  return rc == HYG_OK ? rc : fail(rc, "gather window out of [-1, 256]");
}

int hyg_tg_set_priority_rotation(int32_t on) {
  hyg::tg_set_priority_rotation(on != 0);
  return HYG_OK;
}

int hyg_tg_set_fine_list_walk(int32_t on) {
  hyg::tg_set_fine_list_walk(on != 0);
  return HYG_OK;
}

int32_t hyg_tg_fine_list_walk(void) { return hyg::tg_fine_list_walk(); }

int32_t hyg_tg_priority_base(uint64_t ticks, int32_t slot) { return hyg::tg_priority_base(ticks, slot); }

int32_t hyg_tg_priority_epoch_ticks(void) { return hyg::tg_priority_epoch_ticks(); }

int hyg_tg_set_forward_rounds(int32_t mode) {
  const int rc = hyg::tg_set_forward_rounds(mode);
  return rc == HYG_OK ? rc : fail(rc, "forward rounds out of [0, 2]");
}

int32_t hyg_tg_forward_schedule(const hyg_tg_model* m, const int32_t* n_sites, int32_t n_chains, int32_t multi,
                                int32_t forward_only, int32_t cus, int32_t resident, int32_t max_rounds,
                                int32_t* blocks, int32_t* order, int32_t* begin, int32_t* end) {
  if (!m) return fail(HYG_EINVAL, "null model");
  const int rc = hyg::tg_forward_schedule(m->c, n_sites, n_chains, multi != 0, forward_only != 0, cus, resident,
                                          max_rounds,
                                          blocks, order, begin, end);
  if (rc == HYG_EUNSUPPORTED) return fail_unsupported_shape(m);
  return rc >= 0 ? rc : fail(rc, "forward schedule: null array, no chains, a chain without sites, cus < 0 or max_rounds < 2");
}

int32_t hyg_tg_device_cus(int32_t device) { return hyg::tg_device_cus(device); }

int hyg_tg_set_device_cus(int32_t device, int32_t cus) {
  const int rc = hyg::tg_set_device_cus(device, cus);
  return rc == HYG_OK ? rc : fail(rc, "device out of [0, 64) or negative CU count");
}

int hyg_sg_force_key_drop(int32_t bits) {
  const int rc = hyg::sg_force_key_drop(bits);
  return rc == HYG_OK ? rc : fail(rc, "key bits out of range [8, 60]");
}

int hyg_tg_emission(const hyg_tg_model* m, const uint16_t* meth_c, const uint16_t* tot_c, int32_t s_c,
                    const uint16_t* meth_k, const uint16_t* tot_k, int32_t s_k, int64_t n_sites, double* E,
                    void* stream) {
  if (!m) return fail(HYG_EINVAL, "null model");
  if (!m->on_device) return fail(HYG_EDEVICE, "no HIP device: hygeia_amd has no CPU fallback");
  if (!on_model_device(m->device)) return fail(HYG_EINVAL, "the current HIP device is not the model's device");
  if (s_c < 0 || s_k < 0 || n_sites < 0) return fail(HYG_EINVAL, "negative size");
  if (n_sites > 0 && (!E || (s_c && (!meth_c || !tot_c)) || (s_k && (!meth_k || !tot_k))))
    return fail(HYG_EINVAL, "null buffer");
  return launch_emission(m->dev(), m->c, meth_c, tot_c, s_c, meth_k, tot_k, s_k, n_sites, E, stream);
}

size_t hyg_tg_workspace_bytes(const hyg_tg_model* m, int32_t n_chains, int64_t total_steps) {
  if (!m || n_chains < 0 || total_steps < 0) return 0;
  return header_bytes(n_chains) + (size_t)total_steps * record_bytes(m->c.M) + 256 +
         (size_t)n_chains * chain_scratch_bytes(m->c);
}

size_t hyg_tg_workspace_bytes_multi(const hyg_tg_model* const* models, int32_t n_models, int32_t n_chains,
                                    int64_t total_steps) {
  if (!models || n_models < 1 || !models[0] || n_chains < 0 || total_steps < 0) return 0;
  return hyg_tg_workspace_bytes(models[0], n_chains, total_steps) +
         (header_bytes_multi(n_chains, n_models) - header_bytes(n_chains));
}

// The workspace of a forward-only launch: the header and, for a shape whose
// forward keeps its particle arrays in global memory, each chain's scratch.
size_t hyg_tg_filter_workspace_bytes(const hyg_tg_model* m, int32_t n_chains) {
  if (!m || n_chains < 0) return 0;
  return header_bytes(n_chains) + (size_t)n_chains * filter_scratch_bytes(m->c);
}

size_t hyg_tg_filter_workspace_bytes_multi(const hyg_tg_model* const* models, int32_t n_models, int32_t n_chains) {
  if (!models || n_models < 1 || !models[0] || n_chains < 0) return 0;
  return header_bytes_multi(n_chains, n_models) + (size_t)n_chains * filter_scratch_bytes(models[0]->c);
}

int hyg_tg_models_compatible(const hyg_tg_model* const* models, int32_t n_models) {
  return models_compatible(models, n_models);
}

// ---- the device forms (tg_launch_entry)
int hyg_tg_run_chains(const hyg_tg_model* m, const hyg_tg_chain* chains, int32_t n_chains, const double* E,
                      void* workspace, size_t workspace_bytes, const hyg_tg_outputs* out, void* stream) {
  if (!m) return fail(HYG_EINVAL, "null argument");
  return tg_launch_entry(&m, 1, false, nullptr, chains, n_chains, E, workspace, workspace_bytes, kSmooth, out, nullptr,
                         stream);
}

int hyg_tg_run_chains_multi(const hyg_tg_model* const* models, int32_t n_models, const hyg_tg_chain* chains,
                            const int32_t* chain_model, int32_t n_chains, const double* E, void* workspace,
                            size_t workspace_bytes, const hyg_tg_outputs* out, void* stream) {
  return tg_launch_entry(models, n_models, true, chain_model, chains, n_chains, E, workspace, workspace_bytes, kSmooth,
                         out, nullptr, stream);
}

int hyg_tg_filter_chains(const hyg_tg_model* m, const hyg_tg_chain* chains, int32_t n_chains, const double* E,
                         void* workspace, size_t workspace_bytes, double* log_z, double* final_w, int32_t* status,
                         void* stream) {
  if (!m) return fail(HYG_EINVAL, "null argument");
  const hyg_tg_outputs o = forward_outputs(log_z, final_w, status);
  return tg_launch_entry(&m, 1, false, nullptr, chains, n_chains, E, workspace, workspace_bytes, kFilter, &o, nullptr,
                         stream);
}

int hyg_tg_filter_chains_multi(const hyg_tg_model* const* models, int32_t n_models, const hyg_tg_chain* chains,
                               const int32_t* chain_model, int32_t n_chains, const double* E, void* workspace,
                               size_t workspace_bytes, double* log_z, double* final_w, int32_t* status, void* stream) {
  const hyg_tg_outputs o = forward_outputs(log_z, final_w, status);
  return tg_launch_entry(models, n_models, true, chain_model, chains, n_chains, E, workspace, workspace_bytes, kFilter,
                         &o, nullptr, stream);
}

int hyg_tg_trace_chains(const hyg_tg_model* m, const hyg_tg_chain* chains, int32_t n_chains, const double* E,
                        void* workspace, size_t workspace_bytes, const hyg_tg_trace* trace, double* log_z,
                        double* final_w, int32_t* status, void* stream) {
  if (!m) return fail(HYG_EINVAL, "null argument");
  const hyg_tg_outputs o = forward_outputs(log_z, final_w, status);
  return tg_launch_entry(&m, 1, false, nullptr, chains, n_chains, E, workspace, workspace_bytes, kTrace, &o, trace,
                         stream);
}

int hyg_tg_trace_chains_multi(const hyg_tg_model* const* models, int32_t n_models, const hyg_tg_chain* chains,
                              const int32_t* chain_model, int32_t n_chains, const double* E, void* workspace,
                              size_t workspace_bytes, const hyg_tg_trace* trace, double* log_z, double* final_w,
                              int32_t* status, void* stream) {
  const hyg_tg_outputs o = forward_outputs(log_z, final_w, status);
  return tg_launch_entry(models, n_models, true, chain_model, chains, n_chains, E, workspace, workspace_bytes, kTrace,
                         &o, trace, stream);
}

// ---- the host forms (tg_launch_host)
int hyg_tg_run_chains_host(const hyg_tg_model* m, const uint16_t* meth_c, const uint16_t* tot_c, int32_t s_c,
                           const uint16_t* meth_k, const uint16_t* tot_k, int32_t s_k, int64_t n_sites,
                           const hyg_tg_chain* chains, int32_t n_chains, int64_t out_rows, int16_t* merged,
                           int16_t* control, int16_t* kase, float* split, float* regime, double* log_z,
                           double* final_w, int32_t* status) {
  if (!m) return fail(HYG_EINVAL, "null model");
  return tg_launch_host(&m, 1, false, nullptr, meth_c, tot_c, s_c, meth_k, tot_k, s_k, n_sites, chains, n_chains,
                        kSmooth, {merged, control, kase, split, regime, nullptr, log_z, final_w, status, out_rows});
}

int hyg_tg_run_chains_host_multi(const hyg_tg_model* const* models, int32_t n_models, const uint16_t* meth_c,
                                 const uint16_t* tot_c, int32_t s_c, const uint16_t* meth_k, const uint16_t* tot_k,
                                 int32_t s_k, int64_t n_sites, const hyg_tg_chain* chains,
                                 const int32_t* chain_model, int32_t n_chains, int64_t out_rows, int16_t* merged,
                                 int16_t* control, int16_t* kase, float* split, float* regime, double* log_z,
                                 double* final_w, int32_t* status) {
  return tg_launch_host(models, n_models, true, chain_model, meth_c, tot_c, s_c, meth_k, tot_k, s_k, n_sites, chains,
                        n_chains, kSmooth,
                        {merged, control, kase, split, regime, nullptr, log_z, final_w, status, out_rows});
}

int hyg_tg_filter_chains_host(const hyg_tg_model* m, const uint16_t* meth_c, const uint16_t* tot_c, int32_t s_c,
                              const uint16_t* meth_k, const uint16_t* tot_k, int32_t s_k, int64_t n_sites,
                              const hyg_tg_chain* chains, int32_t n_chains, double* log_z, double* final_w,
                              int32_t* status) {
  if (!m) return fail(HYG_EINVAL, "null model");
  return tg_launch_host(&m, 1, false, nullptr, meth_c, tot_c, s_c, meth_k, tot_k, s_k, n_sites, chains, n_chains,
                        kFilter, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, log_z, final_w, status, 0});
}

int hyg_tg_filter_chains_host_multi(const hyg_tg_model* const* models, int32_t n_models, const uint16_t* meth_c,
                                    const uint16_t* tot_c, int32_t s_c, const uint16_t* meth_k, const uint16_t* tot_k,
                                    int32_t s_k, int64_t n_sites, const hyg_tg_chain* chains,
                                    const int32_t* chain_model, int32_t n_chains, double* log_z, double* final_w,
                                    int32_t* status) {
  return tg_launch_host(models, n_models, true, chain_model, meth_c, tot_c, s_c, meth_k, tot_k, s_k, n_sites, chains,
                        n_chains, kFilter,
                        {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, log_z, final_w, status, 0});
}

int hyg_tg_trace_chains_host(const hyg_tg_model* m, const uint16_t* meth_c, const uint16_t* tot_c, int32_t s_c,
                             const uint16_t* meth_k, const uint16_t* tot_k, int32_t s_k, int64_t n_sites,
                             const hyg_tg_chain* chains, int32_t n_chains, int64_t out_rows, double* log_z_t,
                             float* split, float* regime, double* log_z, double* final_w, int32_t* status) {
  if (!m) return fail(HYG_EINVAL, "null model");
  return tg_launch_host(&m, 1, false, nullptr, meth_c, tot_c, s_c, meth_k, tot_k, s_k, n_sites, chains, n_chains,
                        kTrace, {nullptr, nullptr, nullptr, split, regime, log_z_t, log_z, final_w, status, out_rows});
}

int hyg_tg_trace_chains_host_multi(const hyg_tg_model* const* models, int32_t n_models, const uint16_t* meth_c,
                                   const uint16_t* tot_c, int32_t s_c, const uint16_t* meth_k, const uint16_t* tot_k,
                                   int32_t s_k, int64_t n_sites, const hyg_tg_chain* chains,
                                   const int32_t* chain_model, int32_t n_chains, int64_t out_rows, double* log_z_t,
                                   float* split, float* regime, double* log_z, double* final_w, int32_t* status) {
  return tg_launch_host(models, n_models, true, chain_model, meth_c, tot_c, s_c, meth_k, tot_k, s_k, n_sites, chains,
                        n_chains, kTrace,
                        {nullptr, nullptr, nullptr, split, regime, log_z_t, log_z, final_w, status, out_rows});
}

// ---- the kernel a launch runs (tg_name_impl)
int32_t hyg_tg_kernel_name(const hyg_tg_model* m, int32_t n_chains, int32_t backward, char* buf, int32_t len) {
  if (!m || len < 0) return fail(HYG_EINVAL, "null model or negative length");
  return tg_name_impl(&m, 1, false, backward ? kNameBackward : kNameForward, n_chains, buf, len);
}
int32_t hyg_tg_kernel_name_multi(const hyg_tg_model* const* models, int32_t n_models, int32_t n_chains,
                                 int32_t backward, char* buf, int32_t len) {
  return tg_name_impl(models, n_models, true, backward ? kNameBackward : kNameForward, n_chains, buf, len);
}
int32_t hyg_tg_filter_kernel_name(const hyg_tg_model* m, int32_t n_chains, char* buf, int32_t len) {
  if (!m || len < 0) return fail(HYG_EINVAL, "null model or negative length");
  return tg_name_impl(&m, 1, false, kNameFilter, n_chains, buf, len);
}
int32_t hyg_tg_filter_kernel_name_multi(const hyg_tg_model* const* models, int32_t n_models, int32_t n_chains,
                                        char* buf, int32_t len) {
  return tg_name_impl(models, n_models, true, kNameFilter, n_chains, buf, len);
}
int32_t hyg_tg_trace_kernel_name(const hyg_tg_model* m, int32_t n_chains, char* buf, int32_t len) {
  if (!m || len < 0) return fail(HYG_EINVAL, "null model or negative length");
  return tg_name_impl(&m, 1, false, kNameTrace, n_chains, buf, len);
}
int32_t hyg_tg_trace_kernel_name_multi(const hyg_tg_model* const* models, int32_t n_models, int32_t n_chains,
                                       char* buf, int32_t len) {
  return tg_name_impl(models, n_models, true, kNameTrace, n_chains, buf, len);
}

int hyg_tg_run_chain_host(const hyg_tg_model* m, const uint16_t* meth_c, const uint16_t* tot_c, int32_t s_c,
                          const uint16_t* meth_k, const uint16_t* tot_k, int32_t s_k, int32_t T, uint64_t seed,
                          uint64_t chain_id, int16_t* merged, int16_t* control, int16_t* kase, float* split,
                          float* regime, double* log_z, double* final_w) {
  if (T < 1) return fail(HYG_EINVAL, "no sites");
  hyg_tg_chain ch{};
  ch.site_begin = 0;
  ch.n_sites = T;
  ch.seed = seed;
  ch.chain_id = chain_id;
  ch.out_begin = 0;
  int32_t st = HYG_OK;
  const int rc = hyg_tg_run_chains_host(m, meth_c, tot_c, s_c, meth_k, tot_k, s_k, T, &ch, 1, T, merged, control, kase,
                                        split, regime, log_z, final_w, &st);
  if (rc) return rc;
  if (st != HYG_OK) return fail(st, "all particle weights became -inf");
  return HYG_OK;
}

void hyg_set_kernel_timing(int enable) { set_kernel_timing(enable != 0); }

int hyg_tg_last_kernel_ms(float* ms3) {
  if (!ms3) return fail(HYG_EINVAL, "null argument");
  return last_kernel_ms(ms3);
}

// ============================================================ single group

void hyg_sg_params_default(hyg_sg_params* p) {
  std::memset(p, 0, sizeof(*p));
  // regimes_config defaults (bin/simulate_data:147-157), Beta moments as
  // get_known_parameters (model_functions.R:36-59)
  const double mu[6] = {0.95, 0.05, 0.80, 0.20, 0.50, 0.50};
  const double sg[6] = {0.05, 0.05, 0.1, 0.1, 0.1, 0.2886751};
  const double om[6] = {0.995, 0.975, 0.95, 0.925, 0.9, 0.9};
  p->n_regimes = 6;
  p->minimum_duration = 3;
  p->num_particles_max = 250;
  p->resample_type = 2;
  p->is_kappa_fixed = 1;
  p->theta_len = 36;
  for (int i = 0; i < 6; ++i) {
    const double nu = mu[i] * (1.0 - mu[i]) / (sg[i] * sg[i]) - 1.0;
    p->alpha[i] = mu[i] * nu;
    p->beta[i] = (1.0 - mu[i]) * nu;
    p->kappa[i] = 2.0;
  }
  // uniform off-diagonal transitions (equal log-weights), logit(omega)
  for (int i = 0; i < 30; ++i) p->theta[i] = std::log(1.0 / 5.0);
  for (int i = 0; i < 6; ++i) p->theta[30 + i] = std::log(om[i] / (1.0 - om[i]));
  p->epsilon = 0.01;
}

void hyg_sg_model_destroy(hyg_sg_model* m) {
  if (!m) return;
  if (m->on_device) {
    m->stage.release();
    (void)hipFree(m->d_consts);
    (void)hipFree(m->d_hz);
    (void)hipFree(m->d_ex);
    (void)hipFree(m->d_lf);
    (void)hipFree(m->d_lg);
    (void)hipFree(m->d_cst);
  }
  delete m;
}

int hyg_sg_model_create(const hyg_sg_params* params, int32_t max_total_reads, int32_t max_duration,
                        hyg_sg_model** out) {
  if (!params || !out) return fail(HYG_EINVAL, "null argument");
  *out = nullptr;
  if (max_total_reads < 0 || max_total_reads > 65535) return fail(HYG_EINVAL, "max_total_reads out of [0, 65535]");
  if (max_duration < 1 || max_duration >= HYG_DMAX - 2) return fail(HYG_EINVAL, "max_duration out of range");
  auto* m = new hyg_sg_model();
  int rc = hyg_sg_derive(params, &m->c);
  if (rc != HYG_OK) {
    delete m;
    return fail(rc, rc == HYG_EUNSUPPORTED ? "only resample_type 2 (optimal finite state) is implemented"
                                           : "invalid model parameters");
  }
  if (m->c.Nmax > kSgThreads) {
    delete m;
    return fail(HYG_EUNSUPPORTED, "num_particles_max > 256 (one particle per thread of a workgroup)");
  }
  m->params = *params;
  m->max_duration = max_duration;
  m->nmax_reads = max_total_reads;
  m->dcap = hyg_sg_hazard_len(&m->c, max_duration + 1);
  const int K = m->c.K, L = max_total_reads + 1;
  m->hz.resize((size_t)K * m->dcap * 2);
  m->ex.resize((size_t)K * m->dcap);
  hyg_sg_hazard_fill(&m->c, m->dcap, m->hz.data(), m->ex.data());
  m->lf.resize(L);
  m->lg.resize((size_t)3 * K * L);
  m->cst.resize(K);
  hyg_sg_bb_tables(&m->c, max_total_reads, m->lf.data(), m->lg.data(), m->cst.data());
  if (have_device()) {
    (void)hipGetDevice(&m->device);
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = dmalloc_copy(&m->d_consts, &m->c, 1);
    if (e == hipSuccess) e = dmalloc_copy(&m->d_hz, m->hz.data(), m->hz.size());
    if (e == hipSuccess) e = dmalloc_copy(&m->d_ex, m->ex.data(), m->ex.size());
    if (e == hipSuccess) e = dmalloc_copy(&m->d_lf, m->lf.data(), m->lf.size());
    if (e == hipSuccess) e = dmalloc_copy(&m->d_lg, m->lg.data(), m->lg.size());
    if (e == hipSuccess) e = dmalloc_copy(&m->d_cst, m->cst.data(), m->cst.size());
    m->on_device = true;
    if (e != hipSuccess) {
      hyg_sg_model_destroy(m);
      return fail(HYG_EDEVICE, std::string("device upload failed: ") + hipGetErrorString(e));
    }
  }
  *out = m;
  return HYG_OK;
}

int hyg_sg_emission(const hyg_sg_model* m, const uint16_t* meth, const uint16_t* tot, int32_t n_samples,
                    int64_t n_sites, double* E, void* stream) {
  if (!m) return fail(HYG_EINVAL, "null model");
  if (!m->on_device) return fail(HYG_EDEVICE, "no HIP device: hygeia_amd has no CPU fallback");
  if (!on_model_device(m->device)) return fail(HYG_EINVAL, "the current HIP device is not the model's device");
  if (n_samples < 0 || n_sites < 0) return fail(HYG_EINVAL, "negative size");
  if (n_sites > 0 && (!E || (n_samples && (!meth || !tot)))) return fail(HYG_EINVAL, "null buffer");
  int rc = sg_launch_emission(m->dev(), m->c, meth, tot, n_samples, n_sites, E, stream);
  if (rc != HYG_OK) return fail(rc, "emission launch failed");
  return HYG_OK;
}

}  // extern "C"

// ---------------------------------- single-group host launch layer
// The helpers under hyg_sg_run_chains[_pe][_multi], hyg_sg_{filter,trace}_chains
// [_multi] and their host forms ("Host launch layer").
namespace {

const char kSgUnsupported[] = "particle arrays exceed the LDS of a CU (K too large)";

// workspace header: chain descriptors + status words, then the ring control
// words of every chain (one contiguous block, zeroed before each launch)
size_t sg_desc_bytes(int32_t n_chains) {
  const size_t h = (sizeof(SgChainDev) + sizeof(int32_t)) * (size_t)n_chains;
  return (h + 255) / 256 * 256;
}
size_t sg_header_bytes(int32_t n_chains) {
  return sg_desc_bytes(n_chains) + (kSgCtlBytes * (size_t)n_chains + 255) / 256 * 256;
}

// The header of a multi-model launch: behind the descriptors and the status
// words stand the chain -> model indices (int32 [n_chains]), the model table
// and the per-model estimation inputs (one upload carries all of it); the ring
// control words follow as in sg_header_bytes.
size_t sg_mm_index_offset(int32_t n_chains) { return (sizeof(SgChainDev) + sizeof(int32_t)) * (size_t)n_chains; }
size_t sg_mm_table_offset(int32_t n_chains) {
  return (sg_mm_index_offset(n_chains) + sizeof(int32_t) * (size_t)n_chains + 15) / 16 * 16;
}
size_t sg_mm_upload_bytes(int32_t n_chains, int32_t n_models) {
  return sg_mm_table_offset(n_chains) + (sizeof(SgModelDev) + sizeof(SgPeModelDev)) * (size_t)n_models;
}
size_t sg_desc_bytes_multi(int32_t n_chains, int32_t n_models) {
  return (sg_mm_upload_bytes(n_chains, n_models) + 255) / 256 * 256;
}
size_t sg_header_bytes_multi(int32_t n_chains, int32_t n_models) {
  return sg_desc_bytes_multi(n_chains, n_models) + (kSgCtlBytes * (size_t)n_chains + 255) / 256 * 256;
}

int sg_pe_rcap(int T) { return T + 1 < HYG_SGPE_DCAP ? T + 1 : HYG_SGPE_DCAP; }

// Whether models can share a launch (hyg_sg_models_compatible): the message
// names the first field that differs.
int sg_models_compatible(const hyg_sg_model* const* models, int32_t n_models) {
  if (!models || n_models < 1) return fail(HYG_EINVAL, "no models");
  for (int i = 0; i < n_models; ++i)
    if (!models[i]) return fail(HYG_EINVAL, "null model " + std::to_string(i));
  const hyg_sg_model* a = models[0];
  for (int i = 1; i < n_models; ++i) {
    const hyg_sg_model* b = models[i];
    const char* field = nullptr;
    if (a->params.n_regimes != b->params.n_regimes) field = "n_regimes";
    else if (a->params.minimum_duration != b->params.minimum_duration) field = "minimum_duration";
    else if (a->params.num_particles_max != b->params.num_particles_max) field = "num_particles_max";
    else if ((a->params.is_kappa_fixed != 0) != (b->params.is_kappa_fixed != 0)) field = "is_kappa_fixed";
    else if (a->nmax_reads != b->nmax_reads) field = "max_total_reads";
    else if (std::memcmp(a->params.alpha, b->params.alpha, sizeof(double) * a->c.K) != 0) field = "alpha";
    else if (std::memcmp(a->params.beta, b->params.beta, sizeof(double) * a->c.K) != 0) field = "beta";
    if (field)
      return fail(HYG_EINVAL, std::string("models 0 and ") + std::to_string(i) + " differ in " + field +
                                  ": the models of one launch share the shape and the emission table");
  }
  return HYG_OK;
}

// The read counts of the host forms: tot <= the model's max_total_reads.
int sg_check_counts(const hyg_sg_model* m, const uint16_t* tot, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (tot[i] > m->nmax_reads) return fail(HYG_EINVAL, "total read count above the model's max_total_reads");
  return HYG_OK;
}

// Validates the chains of a launch and fills their descriptors cd[n_chains]
// (zeroed by the caller). chain_model null: every chain runs under models[0].
// desc, header: where the ring control words and the first chain's region
// stand in the workspace (the single-model header's or the _multi one's);
// cap: the psi capacity of a smoothing launch, 0 for a forward-only one, whose
// chains have no region; every: the update interval of a launch with
// estimation (rows and regions are assigned; *max_rows, *max_rcap: the largest
// of a chain), else 0; rows: whether out_begin counts.
int sg_fill_chains(const hyg_sg_model* const* models, const int32_t* chain_model, const hyg_sg_chain* chains,
                   int32_t n_chains, size_t desc, size_t header, int cap, int every, bool rows, SgChainDev* cd,
                   int64_t* max_rows, int* max_rcap) {
  const int K = models[0]->c.K;
  const size_t per = cap ? sg_chain_ws_bytes(K, cap) : 0;
  size_t off = header, pe_off = header + per * (size_t)(n_chains > 0 ? n_chains : 0);
  int64_t row = 0;
  *max_rows = 1;
  *max_rcap = 1;
  for (int i = 0; i < n_chains; ++i) {
    const hyg_sg_chain& c = chains[i];
    if (c.n_sites < 1) return fail(HYG_EINVAL, "chain with no sites");
    if (c.n_sites > models[chain_model ? chain_model[i] : 0]->max_duration)
      return fail(HYG_EINVAL, "chain longer than the model's max_duration");
    if (c.site_begin < 0 || (rows && c.out_begin < 0)) return fail(HYG_EINVAL, "negative chain offset");
    cd[i].site_begin = c.site_begin;
    cd[i].out_begin = rows ? c.out_begin : 0;
    cd[i].seed = c.seed;
    cd[i].chain_id = c.chain_id;
    cd[i].T = c.n_sites;
    if (cap) {  // the psi region, the ring behind it and the control words
      cd[i].psi_offset = (int64_t)off;
      cd[i].ring_offset = (int64_t)(off + sg_psi_region_bytes(K, cap) + sg_lists_bytes(cap));
      cd[i].ctl_offset = (int64_t)(desc + kSgCtlBytes * (size_t)i);
      off += per;
    }
    if (every) {
      cd[i].rcap = sg_pe_rcap(c.n_sites);
      cd[i].pe_offset = (int64_t)pe_off;
      cd[i].theta_row = row;
      const int64_t nr = hyg_sgpe_theta_rows(c.n_sites, every);
      row += nr;
      *max_rows = std::max(*max_rows, nr);
      *max_rcap = std::max(*max_rcap, cd[i].rcap);
      pe_off += sg_pe_region_bytes(K, cd[i].rcap);
    }
  }
  return HYG_OK;
}

// The _multi part of an upload image `up` (zeroed): the chain -> model indices,
// the model table and, with estimation, pem[n_models] behind it. Returns where
// the three will stand on the device, in the workspace ws.
SgMultiDev sg_fill_multi(uint8_t* up, const uint8_t* ws, const hyg_sg_model* const* models, int32_t n_models,
                         const int32_t* chain_model, int32_t n_chains, const SgPeModelDev* pem) {
  const size_t i_off = sg_mm_index_offset(n_chains), t_off = sg_mm_table_offset(n_chains),
               p_off = t_off + sizeof(SgModelDev) * (size_t)n_models;
  std::memcpy(up + i_off, chain_model, sizeof(int32_t) * (size_t)n_chains);
  for (int k = 0; k < n_models; ++k) {
    SgModelDev md = models[k]->dev();
    md.key_keep = sg_key_keep();
    std::memcpy(up + t_off + sizeof(SgModelDev) * (size_t)k, &md, sizeof(SgModelDev));
  }
  if (pem) std::memcpy(up + p_off, pem, sizeof(SgPeModelDev) * (size_t)n_models);
  SgMultiDev mm{};
  mm.models = (const SgModelDev*)(ws + t_off);
  mm.chain_model = (const int32_t*)(ws + i_off);
  mm.pe_models = pem ? (const SgPeModelDev*)(ws + p_off) : nullptr;
  return mm;
}

// hyg_sg_run_chains[_pe] (multi false: the one model models[0], which the entry
// has checked, the single-model header and no SgMultiDev) and
// hyg_sg_run_chains[_pe]_multi. pe == nullptr: no estimation.
int sg_run_chains_impl(const hyg_sg_model* const* models, int32_t n_models, bool multi, const hyg_sg_pe_params* pe,
                       const hyg_sg_chain* chains, const int32_t* chain_model, int32_t n_chains, const double* E,
                       void* workspace, size_t workspace_bytes, int32_t psi_capacity, double* regime_probs,
                       double* theta_out, int32_t* status, void* stream) {
  int rc;
  if (multi) {
    if ((rc = sg_models_compatible(models, n_models)) != HYG_OK) return rc;
    if (n_chains > 0 && (rc = check_chain_models(chain_model, n_chains, n_models)) != HYG_OK) return rc;
  }
  if (!chains || !E || !workspace || !regime_probs || (pe && !theta_out)) return fail(HYG_EINVAL, "null argument");
  if ((rc = models_on_device(models, n_models)) != HYG_OK) return rc;
  if (n_chains <= 0) return HYG_OK;
  if (psi_capacity < 0 || psi_capacity > (1 << 24)) return fail(HYG_EINVAL, "psi_capacity out of range");
  const hyg_sg_model* m = models[0];
  const int K = m->c.K;
  // the estimation settings of every model: they share all but kappa
  std::vector<hyg_sgpe_consts> pcs(pe ? n_models : 0);
  for (int k = 0; pe && k < n_models; ++k)
    if ((rc = hyg_sgpe_consts_make(&models[k]->params, pe, &pcs[k])) != HYG_OK)
      return fail(rc, "invalid parameter-estimation settings");
  const int cap = psi_capacity ? psi_capacity : kSgPsiCapDefault;
  const size_t need =
      multi ? (pe ? hyg_sg_pe_workspace_bytes_multi(models, n_models, chains, n_chains, psi_capacity)
                  : hyg_sg_workspace_bytes_multi(models, n_models, n_chains, psi_capacity))
            : (pe ? hyg_sg_pe_workspace_bytes(m, chains, n_chains, psi_capacity)
                  : hyg_sg_workspace_bytes(m, n_chains, psi_capacity));
  if (workspace_bytes < need)
    return fail(HYG_EINVAL, std::string("workspace too small (see ") +
                                (pe ? "hyg_sg_pe_workspace_bytes" : "hyg_sg_workspace_bytes") + (multi ? "_multi)" : ")"));
  // the upload: the descriptors and, for _multi, the indices and the tables behind them
  const size_t up_bytes = multi ? sg_mm_upload_bytes(n_chains, n_models) : sizeof(SgChainDev) * (size_t)n_chains;
  const size_t desc = multi ? sg_desc_bytes_multi(n_chains, n_models) : sg_desc_bytes(n_chains);
  std::vector<uint8_t> up(up_bytes, 0);
  int64_t max_rows = 1;
  int max_rcap = 1;
  rc = sg_fill_chains(models, multi ? chain_model : nullptr, chains, n_chains, desc,
                      multi ? sg_header_bytes_multi(n_chains, n_models) : sg_header_bytes(n_chains), cap,
                      pe ? pcs[0].every : 0, true, (SgChainDev*)up.data(), &max_rows, &max_rcap);
  if (rc != HYG_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  // estimation inputs: theta0 [n_models][dim] | steps [max_rows] | one lgk (and
  // dgk) table [K][max_rcap] per distinct kappa vector, bit for bit
  AsyncBuf dbuf;
  std::vector<SgPeModelDev> pem(n_models);
  SgPeDev pd{};
  if (pe) {
    const int dim = pcs[0].dim;
    const bool kest = pcs[0].kest != 0;
    std::vector<int> table_of(n_models), first;  // model -> table, table -> its first model
    for (int k = 0; k < n_models; ++k) {
      int t = 0;
      while (t < (int)first.size() && std::memcmp(pcs[first[t]].kappa, pcs[k].kappa, sizeof(double) * K) != 0) ++t;
      if (t == (int)first.size()) first.push_back(k);
      table_of[k] = t;
    }
    const size_t tab = (size_t)K * max_rcap, nt = first.size();
    const size_t b_th = sizeof(double) * dim * (size_t)n_models, b_st = sizeof(hyg_sgpe_step) * (size_t)max_rows,
                 b_lg = sizeof(double) * tab * nt, b_dg = kest ? b_lg : 0;
    std::vector<unsigned char> host(b_th + b_st + b_lg + b_dg);
    for (int k = 0; k < n_models; ++k)
      std::memcpy(host.data() + sizeof(double) * dim * (size_t)k, models[k]->params.theta, sizeof(double) * dim);
    hyg_sgpe_steps_fill(pe, (int)max_rows, (hyg_sgpe_step*)(host.data() + b_th));
    for (size_t t = 0; t < nt; ++t) {
      hyg_sgpe_lgk_fill(pcs[first[t]].kappa, K, max_rcap, (double*)(host.data() + b_th + b_st) + tab * t);
      if (kest)
        hyg_sgpe_dgk_fill(pcs[first[t]].kappa, K, max_rcap, (double*)(host.data() + b_th + b_st + b_lg) + tab * t);
    }
    if (!dbuf.alloc(host.size(), s)) return fail(HYG_ENOMEM, "device allocation failed");
    if (hipMemcpyAsync(dbuf.p, host.data(), host.size(), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return fail(HYG_EDEVICE, "upload failed");
    unsigned char* d = (unsigned char*)dbuf.p;
    for (int k = 0; k < n_models; ++k) {
      pem[k].theta0 = (const double*)d + (size_t)dim * k;
      pem[k].lgk = (const double*)(d + b_th + b_st) + tab * table_of[k];
      pem[k].dgk = kest ? (const double*)(d + b_th + b_st + b_lg) + tab * table_of[k] : nullptr;
    }
    pd.c = pcs[0];
    pd.theta0 = pem[0].theta0;
    pd.steps = (const hyg_sgpe_step*)(d + b_th);
    pd.lgk = pem[0].lgk;
    pd.dgk = pem[0].dgk;
    pd.lgk_stride = max_rcap;
    pd.theta_out = theta_out;
  }
  SgMultiDev mm{};
  if (multi) mm = sg_fill_multi(up.data(), ws, models, n_models, chain_model, n_chains, pe ? pem.data() : nullptr);
  if (m->stage.upload(ws, up.data(), up_bytes, s) != hipSuccess) return fail(HYG_EDEVICE, "descriptor upload failed");
  int32_t* st = status ? status : (int32_t*)(ws + sizeof(SgChainDev) * n_chains);
  rc = sg_launch_chains(m->dev(), m->c, (const SgChainDev*)ws, n_chains, E, ws, cap, regime_probs, st, ws + desc,
                        stream, pe ? &pd : nullptr, multi ? &mm : nullptr);
  return launch_result(rc, kSgUnsupported);
}

// hyg_sg_run_chain_host (pe and theta_out null) and hyg_sg_run_chain_host_pe,
// which have refused their null arguments: the one chain of all T sites, its
// status the call's code.
int sg_run_chain_host_impl(const hyg_sg_model* m, const hyg_sg_pe_params* pe, const uint16_t* meth,
                           const uint16_t* tot, int32_t S, int32_t T, uint64_t seed, uint64_t chain_id,
                           double* regime_probs, double* theta_out) {
  int rc;
  if ((rc = models_on_device(&m, 1)) != HYG_OK) return rc;
  if (T < 1 || S < 0) return fail(HYG_EINVAL, "no sites");
  if (pe && pe->n_steps_without_update < 1) return fail(HYG_EINVAL, "n_steps_without_update < 1");
  if ((rc = sg_check_counts(m, tot, (int64_t)T * S)) != HYG_OK) return rc;
  const int K = m->c.K;
  hyg_sg_chain ch{};  // (site_begin and out_begin 0)
  ch.n_sites = T;
  ch.seed = seed;
  ch.chain_id = chain_id;
  const size_t nc = (size_t)T * S, pb = sizeof(double) * T * K;
  const size_t wsb = pe ? hyg_sg_pe_workspace_bytes(m, &ch, 1, 0) : hyg_sg_workspace_bytes(m, 1, 0);
  const int dth = m->params.is_kappa_fixed ? K * K : K * (K + 1);
  const size_t thb = pe ? sizeof(double) * (size_t)hyg_sgpe_theta_rows(T, pe->n_steps_without_update) * dth : 0;
  DevBuf b_m, b_t, b_E, b_ws, b_p, b_st, b_th;
  if (!b_m.alloc(nc * 2) || !b_t.alloc(nc * 2) || !b_E.alloc(pb) || !b_ws.alloc(wsb) || !b_p.alloc(pb) ||
      !b_st.alloc(4) || !b_th.alloc_for(theta_out, thb))
    return fail(HYG_ENOMEM, "device allocation failed");
  if (!b_m.upload(meth, nc * 2) || !b_t.upload(tot, nc * 2)) return fail(HYG_EDEVICE, "copy failed");
  rc = hyg_sg_emission(m, (uint16_t*)b_m.p, (uint16_t*)b_t.p, S, T, (double*)b_E.p, nullptr);
  if (rc) return rc;
  rc = sg_run_chains_impl(&m, 1, false, pe, &ch, nullptr, 1, (double*)b_E.p, b_ws.p, wsb, 0, (double*)b_p.p,
                          (double*)b_th.p, (int32_t*)b_st.p, nullptr);
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(HYG_EDEVICE, "kernel execution failed");
  int32_t st = 0;
  if (!b_st.download(&st, 4) || !b_p.download(regime_probs, pb) || !b_th.download(theta_out, thb))
    return fail(HYG_EDEVICE, "copy failed");
  if (st == HYG_ENOMEM)
    return fail(st, pe ? "pending smoothing times exceeded psi_capacity, or a sojourn outgrew the hazard rows"
                       : "pending smoothing times exceeded psi_capacity");
  if (st != HYG_OK) return fail(st, "all particle weights became -inf");
  return HYG_OK;
}

// All eight forward-only device entries. multi false: the single-model builds
// (n_models is 1). traced: `trace` must name at least one array. Every refusal
// that needs no device comes before the device check, and nothing is enqueued
// before the last of them.
int sg_filter_impl(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                   const int32_t* chain_model, bool multi, int32_t n_chains, const double* E, void* workspace,
                   size_t workspace_bytes, bool traced, const hyg_sg_trace* trace, double* log_z, double* final_lw,
                   int32_t* final_st, int32_t* n_part, int32_t* status, void* stream, bool with_history = false,
                   const hyg_sg_history* history = nullptr) {
  int rc = sg_models_compatible(models, n_models);
  if (rc != HYG_OK) return rc;
  if (multi && n_chains > 0 && (rc = check_chain_models(chain_model, n_chains, n_models)) != HYG_OK) return rc;
  if (!chains || !E || !workspace || !log_z) return fail(HYG_EINVAL, "null argument");
  if (traced && (!trace || (!trace->log_z_t && !trace->regime_probs && !trace->cp_probs)))
    return fail(HYG_EINVAL, "null trace: hyg_sg_trace_chains needs at least one of log_z_t, regime_probs, cp_probs");
  if (with_history && (!history || !history->log_weights || !history->states || !history->n_particles))
    return fail(HYG_EINVAL, "null history: hyg_sg_history_chains_multi needs log_weights, states and n_particles");
  const hyg_sg_model* m = models[0];
  // the upload: the descriptors (no regions: the workspace is its header) and, for _multi, indices and model table
  const size_t up_bytes =
      n_chains <= 0 ? 0 : multi ? sg_mm_upload_bytes(n_chains, n_models) : sizeof(SgChainDev) * (size_t)n_chains;
  std::vector<uint8_t> up(up_bytes, 0);
  int64_t max_rows;
  int max_rcap;
  rc = sg_fill_chains(models, multi ? chain_model : nullptr, chains, n_chains, 0, 0, 0, 0, traced || with_history,
                      (SgChainDev*)up.data(), &max_rows, &max_rcap);
  if (rc != HYG_OK) return rc;
  const size_t need = multi ? hyg_sg_filter_workspace_bytes_multi(models, n_models, n_chains)
                            : hyg_sg_filter_workspace_bytes(m, n_chains);
  if (workspace_bytes < need)
    return fail(HYG_EINVAL, multi ? "workspace too small (see hyg_sg_filter_workspace_bytes_multi)"
                                  : "workspace too small (see hyg_sg_filter_workspace_bytes)");
  const char* name = nullptr;
  if (sg_filter_kernel_name(m->c, multi, traced, &name) != HYG_OK) return fail(HYG_EUNSUPPORTED, kSgUnsupported);
  if ((rc = models_on_device(models, n_models)) != HYG_OK) return rc;
  if (n_chains <= 0) return HYG_OK;
  uint8_t* ws = (uint8_t*)workspace;
  SgMultiDev mm{};
  if (multi) mm = sg_fill_multi(up.data(), ws, models, n_models, chain_model, n_chains, nullptr);
  if (m->stage.upload(ws, up.data(), up_bytes, (hipStream_t)stream) != hipSuccess)
    return fail(HYG_EDEVICE, "descriptor upload failed");
  SgFoDev out{};
  out.log_z = log_z;
  out.final_lw = final_lw;
  out.final_st = final_st;
  out.n_part = n_part;
  if (traced) {
    out.log_z_t = trace->log_z_t;
    out.regime_probs = trace->regime_probs;
    out.cp_probs = trace->cp_probs;
  }
  int32_t* st = status ? status : (int32_t*)(ws + sizeof(SgChainDev) * n_chains);
  if (with_history) {  // (multi only: the history builds exist in the multi-model form)
    SgHistDev hd{};
    hd.lw = history->log_weights;
    hd.st = history->states;
    hd.n_part = history->n_particles;
    rc = sg_launch_history_multi(mm, m->c, (const SgChainDev*)ws, n_chains, E, ws, out, hd, st, stream);
  } else {
    rc = sg_launch_filter(m->dev(), m->c, (const SgChainDev*)ws, n_chains, E, ws, out, traced, st, stream,
                          multi ? &mm : nullptr);
  }
  return launch_result(rc, kSgUnsupported);
}

// The two forward-only host forms: out_rows < 0 is the untraced one.
int sg_filter_host_impl(const hyg_sg_model* const* models, int32_t n_models, const uint16_t* meth, const uint16_t* tot,
                        int32_t S, int64_t n_sites, const hyg_sg_chain* chains, const int32_t* chain_model,
                        int32_t n_chains, bool traced, int64_t out_rows, double* log_z_t, double* regime_probs,
                        double* cp_probs, double* log_z, double* final_lw, int32_t* final_st, int32_t* n_part,
                        int32_t* status) {
  int rc = sg_models_compatible(models, n_models);
  if (rc != HYG_OK) return rc;
  const hyg_sg_model* m = models[0];
  if (n_chains < 1) return fail(HYG_EINVAL, "empty or negative size");
  if ((rc = check_chain_models(chain_model, n_chains, n_models)) != HYG_OK) return rc;
  if (n_sites < 1 || S < 0 || (traced && out_rows < 1)) return fail(HYG_EINVAL, "empty or negative size");
  if (!chains || !log_z || !status || (S > 0 && (!meth || !tot))) return fail(HYG_EINVAL, "null argument");
  if (traced && !log_z_t && !regime_probs && !cp_probs)
    return fail(HYG_EINVAL, "null trace: hyg_sg_trace_chains needs at least one of log_z_t, regime_probs, cp_probs");
  for (int i = 0; i < n_chains; ++i) {
    const hyg_sg_chain& c = chains[i];
    if (c.n_sites < 1 || c.site_begin < 0 || c.site_begin + c.n_sites > n_sites ||
        (traced && (c.out_begin < 0 || c.out_begin + c.n_sites > out_rows)))
      return fail(HYG_EINVAL, "chain outside the sites or the output rows");
    if (c.n_sites > models[chain_model[i]]->max_duration)
      return fail(HYG_EINVAL, "chain longer than the model's max_duration");
  }
  if ((rc = models_on_device(models, n_models)) != HYG_OK) return rc;
  if ((rc = sg_check_counts(m, tot, n_sites * S)) != HYG_OK) return rc;
  const size_t K = m->c.K, Nmax = m->c.Nmax;
  DevBuf b_m, b_t, b_E, b_ws, b_z, b_lw, b_fs, b_np, b_st, b_zt, b_rp, b_cp;
  const size_t nc = (size_t)n_sites * S, nch = (size_t)n_chains, rows = traced ? (size_t)out_rows : 0;
  const size_t wsb = hyg_sg_filter_workspace_bytes_multi(models, n_models, n_chains);
  const bool ok = b_m.alloc(nc * 2) && b_t.alloc(nc * 2) && b_E.alloc(sizeof(double) * (size_t)n_sites * K) &&
                  b_ws.alloc(wsb) && b_z.alloc(8 * nch) && b_st.alloc(4 * nch) &&
                  b_lw.alloc_for(final_lw, 8 * nch * Nmax) && b_fs.alloc_for(final_st, 8 * nch * Nmax) &&
                  b_np.alloc_for(n_part, 4 * nch) && b_zt.alloc_for(log_z_t, 8 * rows) &&
                  b_rp.alloc_for(regime_probs, 8 * rows * K) && b_cp.alloc_for(cp_probs, 8 * rows);
  if (!ok) return fail(HYG_ENOMEM, "device allocation failed");
  // rows of the trace that no chain owns keep the caller's values
  if (!b_m.upload(meth, nc * 2) || !b_t.upload(tot, nc * 2) || !b_zt.upload(log_z_t, 8 * rows) ||
      !b_rp.upload(regime_probs, 8 * rows * K) || !b_cp.upload(cp_probs, 8 * rows))
    return fail(HYG_EDEVICE, "copy failed");
  rc = hyg_sg_emission(m, (uint16_t*)b_m.p, (uint16_t*)b_t.p, S, n_sites, (double*)b_E.p, nullptr);
  if (rc) return rc;
  hyg_sg_trace tr{};
  tr.log_z_t = (double*)b_zt.p;
  tr.regime_probs = (double*)b_rp.p;
  tr.cp_probs = (double*)b_cp.p;
  rc = sg_filter_impl(models, n_models, chains, chain_model, true, n_chains, (double*)b_E.p, b_ws.p, wsb, traced, &tr,
                      (double*)b_z.p, (double*)b_lw.p, (int32_t*)b_fs.p, (int32_t*)b_np.p, (int32_t*)b_st.p, nullptr);
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(HYG_EDEVICE, "kernel execution failed");
  if (!b_st.download(status, 4 * nch) || !b_z.download(log_z, 8 * nch) || !b_lw.download(final_lw, 8 * nch * Nmax) ||
      !b_fs.download(final_st, 8 * nch * Nmax) || !b_np.download(n_part, 4 * nch) ||
      !b_zt.download(log_z_t, 8 * rows) || !b_rp.download(regime_probs, 8 * rows * K) ||
      !b_cp.download(cp_probs, 8 * rows))
    return fail(HYG_EDEVICE, "copy failed");
  return HYG_OK;
}

// hyg_sg_sample_paths_multi: the refusals of the forward-only entries in their
// order, the descriptors and the model table in a stream-ordered side
// allocation (the entry takes no workspace), one launch.
int sg_sample_impl(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                   const int32_t* chain_model, int32_t n_chains, const hyg_sg_history* history,
                   const int32_t* forward_status, int32_t B, int16_t* paths, int32_t* sample_status, void* stream) {
  int rc = sg_models_compatible(models, n_models);
  if (rc != HYG_OK) return rc;
  if (n_chains > 0 && (rc = check_chain_models(chain_model, n_chains, n_models)) != HYG_OK) return rc;
  if (!chains || !paths) return fail(HYG_EINVAL, "null argument");
  if (!history || !history->log_weights || !history->states || !history->n_particles)
    return fail(HYG_EINVAL, "null history: hyg_sg_sample_paths_multi needs log_weights, states and n_particles");
  if (B < 1 || B > 1024) return fail(HYG_EINVAL, "n_trajectories outside [1, 1024]");
  const hyg_sg_model* m = models[0];
  const size_t up_bytes = n_chains <= 0 ? 0 : sg_mm_upload_bytes(n_chains, n_models);
  std::vector<uint8_t> up(up_bytes, 0);
  int64_t max_rows;
  int max_rcap;
  rc = sg_fill_chains(models, chain_model, chains, n_chains, 0, 0, 0, 0, true, (SgChainDev*)up.data(), &max_rows,
                      &max_rcap);
  if (rc != HYG_OK) return rc;
  if (m->c.Nmax > kSgThreads) return fail(HYG_EUNSUPPORTED, kSgUnsupported);
  if ((rc = models_on_device(models, n_models)) != HYG_OK) return rc;
  if (n_chains <= 0) return HYG_OK;
  AsyncBuf side;
  if (!side.alloc(up_bytes, (hipStream_t)stream))
    return fail(HYG_ENOMEM, "device allocation failed (" + std::to_string(up_bytes) + " bytes)");
  uint8_t* ws = (uint8_t*)side.p;
  const SgMultiDev mm = sg_fill_multi(up.data(), ws, models, n_models, chain_model, n_chains, nullptr);
  if (m->stage.upload(ws, up.data(), up_bytes, (hipStream_t)stream) != hipSuccess)
    return fail(HYG_EDEVICE, "descriptor upload failed");
  SgHistDev hd{};
  hd.lw = history->log_weights;
  hd.st = history->states;
  hd.n_part = history->n_particles;
  rc = sg_launch_sample(mm, m->c, (const SgChainDev*)ws, n_chains, hd, forward_status, B, paths, sample_status,
                        stream);
  return launch_result(rc, kSgUnsupported);
}

// hyg_sg_sample_chains_host_multi: the refusals of sg_filter_host_impl's traced
// form, then both stages on the default stream.
int sg_sample_host_impl(const hyg_sg_model* const* models, int32_t n_models, const uint16_t* meth, const uint16_t* tot,
                        int32_t S, int64_t n_sites, const hyg_sg_chain* chains, const int32_t* chain_model,
                        int32_t n_chains, int32_t B, int64_t out_rows, int16_t* paths, double* log_z,
                        int32_t* status) {
  int rc = sg_models_compatible(models, n_models);
  if (rc != HYG_OK) return rc;
  const hyg_sg_model* m = models[0];
  if (n_chains < 1) return fail(HYG_EINVAL, "empty or negative size");
  if ((rc = check_chain_models(chain_model, n_chains, n_models)) != HYG_OK) return rc;
  if (n_sites < 1 || S < 0 || out_rows < 1) return fail(HYG_EINVAL, "empty or negative size");
  if (B < 1 || B > 1024) return fail(HYG_EINVAL, "n_trajectories outside [1, 1024]");
  if (!chains || !paths || !log_z || !status || (S > 0 && (!meth || !tot))) return fail(HYG_EINVAL, "null argument");
  for (int i = 0; i < n_chains; ++i) {
    const hyg_sg_chain& c = chains[i];
    if (c.n_sites < 1 || c.site_begin < 0 || c.site_begin + c.n_sites > n_sites || c.out_begin < 0 ||
        c.out_begin + c.n_sites > out_rows)
      return fail(HYG_EINVAL, "chain outside the sites or the output rows");
    if (c.n_sites > models[chain_model[i]]->max_duration)
      return fail(HYG_EINVAL, "chain longer than the model's max_duration");
  }
  if ((rc = models_on_device(models, n_models)) != HYG_OK) return rc;
  if ((rc = sg_check_counts(m, tot, n_sites * S)) != HYG_OK) return rc;
  const size_t K = m->c.K, Nmax = m->c.Nmax;
  const size_t nc = (size_t)n_sites * S, nch = (size_t)n_chains, rows = (size_t)out_rows;
  const size_t wsb = hyg_sg_filter_workspace_bytes_multi(models, n_models, n_chains);
  const size_t eb = sizeof(double) * (size_t)n_sites * K, pb = 4 * rows * (size_t)B;
  const size_t hb = 12 * rows * Nmax + 4 * rows;
  DevBuf b_m, b_t, b_E, b_ws, b_z, b_st, b_hl, b_hs, b_hn, b_p;
  const bool ok = b_m.alloc(nc * 2) && b_t.alloc(nc * 2) && b_E.alloc(eb) && b_ws.alloc(wsb) && b_z.alloc(8 * nch) &&
                  b_st.alloc(4 * nch) && b_hl.alloc(8 * rows * Nmax) && b_hs.alloc(4 * rows * Nmax) &&
                  b_hn.alloc(4 * rows) && b_p.alloc(pb);
  if (!ok)
    return fail(HYG_ENOMEM, "device allocation failed: " + std::to_string(4 * nc + eb + wsb + 12 * nch + hb + pb) +
                                " bytes asked for (" + std::to_string(hb) + " of them the history)");
  // rows of the paths that no chain owns keep the caller's values
  if (!b_m.upload(meth, nc * 2) || !b_t.upload(tot, nc * 2) || !b_p.upload(paths, pb))
    return fail(HYG_EDEVICE, "copy failed");
  rc = hyg_sg_emission(m, (uint16_t*)b_m.p, (uint16_t*)b_t.p, S, n_sites, (double*)b_E.p, nullptr);
  if (rc) return rc;
  hyg_sg_history hist{};
  hist.log_weights = (double*)b_hl.p;
  hist.states = (uint32_t*)b_hs.p;
  hist.n_particles = (int32_t*)b_hn.p;
  rc = sg_filter_impl(models, n_models, chains, chain_model, true, n_chains, (double*)b_E.p, b_ws.p, wsb, false,
                      nullptr, (double*)b_z.p, nullptr, nullptr, nullptr, (int32_t*)b_st.p, nullptr, true, &hist);
  if (rc) return rc;
  rc = sg_sample_impl(models, n_models, chains, chain_model, n_chains, &hist, (const int32_t*)b_st.p, B,
                      (int16_t*)b_p.p, nullptr, nullptr);
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(HYG_EDEVICE, "kernel execution failed");
  if (!b_st.download(status, 4 * nch) || !b_z.download(log_z, 8 * nch) || !b_p.download(paths, pb))
    return fail(HYG_EDEVICE, "copy failed");
  return HYG_OK;
}

int32_t sg_filter_name_impl(const hyg_sg_model* const* models, int32_t n_models, bool multi, bool trace, char* buf,
                            int32_t len) {
  if (len < 0) return fail(HYG_EINVAL, "negative length");
  const int rc = sg_models_compatible(models, n_models);
  if (rc != HYG_OK) return rc;
  const char* name = nullptr;
  if (sg_filter_kernel_name(models[0]->c, multi, trace, &name) != HYG_OK)
    return fail(HYG_EUNSUPPORTED, kSgUnsupported);
  return copy_name(name, buf, len);
}

}  // namespace

extern "C" {

size_t hyg_sg_workspace_bytes(const hyg_sg_model* m, int32_t n_chains, int32_t psi_capacity) {
  if (!m || n_chains < 0 || psi_capacity < 0) return 0;
  const int cap = psi_capacity ? psi_capacity : kSgPsiCapDefault;
  return sg_header_bytes(n_chains) + (size_t)n_chains * sg_chain_ws_bytes(m->c.K, cap);
}

// ---- online parameter estimation

void hyg_sg_pe_params_default(hyg_sg_pe_params* pe) {
  std::memset(pe, 0, sizeof(*pe));
  // bin/estimate_parameters_and_regimes:130-200 flag defaults
  pe->use_adam = 1;
  pe->normalise_gradients = 0;
  pe->n_steps_without_update = 200;
  pe->learning_rate_exponent = 0.1;
  pe->learning_rate_factor = 0.01;
}

int64_t hyg_sg_pe_theta_rows(const hyg_sg_chain* chains, int32_t n_chains, int32_t every) {
  if (!chains || n_chains < 0 || every < 1) return -1;
  int64_t rows = 0;
  for (int i = 0; i < n_chains; ++i) rows += hyg_sgpe_theta_rows(chains[i].n_sites, every);
  return rows;
}

size_t hyg_sg_pe_workspace_bytes(const hyg_sg_model* m, const hyg_sg_chain* chains, int32_t n_chains,
                                 int32_t psi_capacity) {
  if (!m || !chains || n_chains < 0 || psi_capacity < 0) return 0;
  size_t b = hyg_sg_workspace_bytes(m, n_chains, psi_capacity);
  for (int i = 0; i < n_chains; ++i) b += sg_pe_region_bytes(m->c.K, sg_pe_rcap(std::max(chains[i].n_sites, 1)));
  return b;
}

int hyg_sg_run_chains(const hyg_sg_model* m, const hyg_sg_chain* chains, int32_t n_chains, const double* E,
                      void* workspace, size_t workspace_bytes, int32_t psi_capacity, double* regime_probs,
                      int32_t* status, void* stream) {
  if (!m) return fail(HYG_EINVAL, "null argument");
  return sg_run_chains_impl(&m, 1, false, nullptr, chains, nullptr, n_chains, E, workspace, workspace_bytes,
                            psi_capacity, regime_probs, nullptr, status, stream);
}

int hyg_sg_run_chains_pe(const hyg_sg_model* m, const hyg_sg_pe_params* pe, const hyg_sg_chain* chains,
                         int32_t n_chains, const double* E, void* workspace, size_t workspace_bytes,
                         int32_t psi_capacity, double* regime_probs, double* theta_out, int32_t* status,
                         void* stream) {
  if (!m || !pe) return fail(HYG_EINVAL, "null argument");
  return sg_run_chains_impl(&m, 1, false, pe, chains, nullptr, n_chains, E, workspace, workspace_bytes, psi_capacity,
                            regime_probs, theta_out, status, stream);
}

int hyg_sg_run_chain_host(const hyg_sg_model* m, const uint16_t* meth, const uint16_t* tot, int32_t S, int32_t T,
                          uint64_t seed, uint64_t chain_id, double* regime_probs) {
  if (!m || !regime_probs || (S > 0 && (!meth || !tot))) return fail(HYG_EINVAL, "null argument");
  return sg_run_chain_host_impl(m, nullptr, meth, tot, S, T, seed, chain_id, regime_probs, nullptr);
}

int hyg_sg_run_chain_host_pe(const hyg_sg_model* m, const hyg_sg_pe_params* pe, const uint16_t* meth,
                             const uint16_t* tot, int32_t S, int32_t T, uint64_t seed, uint64_t chain_id,
                             double* regime_probs, double* theta_out) {
  if (!m || !pe || !regime_probs || !theta_out || (S > 0 && (!meth || !tot))) return fail(HYG_EINVAL, "null argument");
  return sg_run_chain_host_impl(m, pe, meth, tot, S, T, seed, chain_id, regime_probs, theta_out);
}

// ---- multi-model launches: chain i runs under models[chain_model[i]]

int hyg_sg_models_compatible(const hyg_sg_model* const* models, int32_t n_models) {
  return sg_models_compatible(models, n_models);
}

size_t hyg_sg_workspace_bytes_multi(const hyg_sg_model* const* models, int32_t n_models, int32_t n_chains,
                                    int32_t psi_capacity) {
  if (!models || n_models < 1 || !models[0] || n_chains < 0 || psi_capacity < 0) return 0;
  return hyg_sg_workspace_bytes(models[0], n_chains, psi_capacity) +
         (sg_header_bytes_multi(n_chains, n_models) - sg_header_bytes(n_chains));
}

size_t hyg_sg_pe_workspace_bytes_multi(const hyg_sg_model* const* models, int32_t n_models,
                                       const hyg_sg_chain* chains, int32_t n_chains, int32_t psi_capacity) {
  if (!models || n_models < 1 || !models[0] || !chains || n_chains < 0 || psi_capacity < 0) return 0;
  return hyg_sg_pe_workspace_bytes(models[0], chains, n_chains, psi_capacity) +
         (sg_header_bytes_multi(n_chains, n_models) - sg_header_bytes(n_chains));
}

int hyg_sg_run_chains_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                            const int32_t* chain_model, int32_t n_chains, const double* E, void* workspace,
                            size_t workspace_bytes, int32_t psi_capacity, double* regime_probs, int32_t* status,
                            void* stream) {
  return sg_run_chains_impl(models, n_models, true, nullptr, chains, chain_model, n_chains, E, workspace,
                            workspace_bytes, psi_capacity, regime_probs, nullptr, status, stream);
}

int hyg_sg_run_chains_pe_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_pe_params* pe,
                               const hyg_sg_chain* chains, const int32_t* chain_model, int32_t n_chains,
                               const double* E, void* workspace, size_t workspace_bytes, int32_t psi_capacity,
                               double* regime_probs, double* theta_out, int32_t* status, void* stream) {
  if (!pe) return fail(HYG_EINVAL, "null argument");
  return sg_run_chains_impl(models, n_models, true, pe, chains, chain_model, n_chains, E, workspace, workspace_bytes,
                            psi_capacity, regime_probs, theta_out, status, stream);
}

int hyg_sg_run_chains_host_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_pe_params* pe,
                                 const uint16_t* meth, const uint16_t* tot, int32_t S, int64_t n_sites,
                                 const hyg_sg_chain* chains, const int32_t* chain_model, int32_t n_chains,
                                 int64_t out_rows, double* regime_probs, double* theta_out, int32_t* status) {
  int rc = sg_models_compatible(models, n_models);
  if (rc != HYG_OK) return rc;
  const hyg_sg_model* m = models[0];
  if (n_chains < 1) return fail(HYG_EINVAL, "empty or negative size");
  if ((rc = check_chain_models(chain_model, n_chains, n_models)) != HYG_OK) return rc;
  if ((rc = models_on_device(models, n_models)) != HYG_OK) return rc;
  if (n_sites < 1 || out_rows < 1 || S < 0) return fail(HYG_EINVAL, "empty or negative size");
  if (!chains || !regime_probs || !status || (pe && !theta_out) || (S > 0 && (!meth || !tot)))
    return fail(HYG_EINVAL, "null argument");
  if (pe && pe->n_steps_without_update < 1) return fail(HYG_EINVAL, "n_steps_without_update < 1");
  for (int i = 0; i < n_chains; ++i) {
    const hyg_sg_chain& c = chains[i];
    if (c.n_sites < 1 || c.site_begin < 0 || c.out_begin < 0 || c.site_begin + c.n_sites > n_sites ||
        c.out_begin + c.n_sites > out_rows)
      return fail(HYG_EINVAL, "chain outside the sites or the output rows");
  }
  if ((rc = sg_check_counts(m, tot, n_sites * S)) != HYG_OK) return rc;
  const size_t K = m->c.K;
  DevBuf b_m, b_t, b_E, b_ws, b_p, b_st, b_th;
  const size_t nc = (size_t)n_sites * S, nch = (size_t)n_chains;
  const size_t wsb = pe ? hyg_sg_pe_workspace_bytes_multi(models, n_models, chains, n_chains, 0)
                        : hyg_sg_workspace_bytes_multi(models, n_models, n_chains, 0);
  const int dth = m->params.is_kappa_fixed ? (int)(K * K) : (int)(K * (K + 1));
  const size_t thb =
      pe ? sizeof(double) * (size_t)hyg_sg_pe_theta_rows(chains, n_chains, pe->n_steps_without_update) * dth : 0;
  const size_t pb = sizeof(double) * (size_t)out_rows * K;
  if (!b_m.alloc(nc * 2) || !b_t.alloc(nc * 2) || !b_E.alloc(sizeof(double) * (size_t)n_sites * K) ||
      !b_ws.alloc(wsb) || !b_p.alloc(pb) || !b_st.alloc(4 * nch) || !b_th.alloc(thb))
    return fail(HYG_ENOMEM, "device allocation failed");
  if (!b_m.upload(meth, nc * 2) || !b_t.upload(tot, nc * 2)) return fail(HYG_EDEVICE, "copy failed");
  // rows of the output that no chain covers stay 0
  if (hipMemset(b_p.p, 0, pb) != hipSuccess) return fail(HYG_EDEVICE, "copy failed");
  rc = hyg_sg_emission(m, (uint16_t*)b_m.p, (uint16_t*)b_t.p, S, n_sites, (double*)b_E.p, nullptr);
  if (rc) return rc;
  rc = sg_run_chains_impl(models, n_models, true, pe, chains, chain_model, n_chains, (double*)b_E.p, b_ws.p, wsb, 0,
                          (double*)b_p.p, (double*)b_th.p, (int32_t*)b_st.p, nullptr);
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(HYG_EDEVICE, "kernel execution failed");
  if (!b_st.download(status, 4 * nch) || !b_p.download(regime_probs, pb) || !b_th.download(theta_out, thb))
    return fail(HYG_EDEVICE, "copy failed");
  return HYG_OK;
}

// ---- forward-only launches (hyg_sg_filter_chains, hyg_sg_trace_chains)

// The workspace of a forward-only launch is its header: descriptors and status
// words, for _multi the chain -> model indices and the model table behind them.
size_t hyg_sg_filter_workspace_bytes(const hyg_sg_model* m, int32_t n_chains) {
  if (!m || n_chains < 0) return 0;
  return sg_desc_bytes(n_chains);
}

size_t hyg_sg_filter_workspace_bytes_multi(const hyg_sg_model* const* models, int32_t n_models, int32_t n_chains) {
  if (!models || n_models < 1 || !models[0] || n_chains < 0) return 0;
  return sg_desc_bytes_multi(n_chains, n_models);
}

int hyg_sg_filter_chains(const hyg_sg_model* m, const hyg_sg_chain* chains, int32_t n_chains, const double* E,
                         void* workspace, size_t workspace_bytes, double* log_z, double* final_lw, int32_t* final_st,
                         int32_t* n_part, int32_t* status, void* stream) {
  if (!m) return fail(HYG_EINVAL, "null argument");
  return sg_filter_impl(&m, 1, chains, nullptr, false, n_chains, E, workspace, workspace_bytes, false, nullptr, log_z,
                        final_lw, final_st, n_part, status, stream);
}

int hyg_sg_filter_chains_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                               const int32_t* chain_model, int32_t n_chains, const double* E, void* workspace,
                               size_t workspace_bytes, double* log_z, double* final_lw, int32_t* final_st,
                               int32_t* n_part, int32_t* status, void* stream) {
  return sg_filter_impl(models, n_models, chains, chain_model, true, n_chains, E, workspace, workspace_bytes, false,
                        nullptr, log_z, final_lw, final_st, n_part, status, stream);
}

int hyg_sg_trace_chains(const hyg_sg_model* m, const hyg_sg_chain* chains, int32_t n_chains, const double* E,
                        void* workspace, size_t workspace_bytes, const hyg_sg_trace* trace, double* log_z,
                        double* final_lw, int32_t* final_st, int32_t* n_part, int32_t* status, void* stream) {
  if (!m) return fail(HYG_EINVAL, "null argument");
  return sg_filter_impl(&m, 1, chains, nullptr, false, n_chains, E, workspace, workspace_bytes, true, trace, log_z,
                        final_lw, final_st, n_part, status, stream);
}

int hyg_sg_trace_chains_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                              const int32_t* chain_model, int32_t n_chains, const double* E, void* workspace,
                              size_t workspace_bytes, const hyg_sg_trace* trace, double* log_z, double* final_lw,
                              int32_t* final_st, int32_t* n_part, int32_t* status, void* stream) {
  return sg_filter_impl(models, n_models, chains, chain_model, true, n_chains, E, workspace, workspace_bytes, true,
                        trace, log_z, final_lw, final_st, n_part, status, stream);
}

int hyg_sg_filter_chains_host_multi(const hyg_sg_model* const* models, int32_t n_models, const uint16_t* meth,
                                    const uint16_t* tot, int32_t S, int64_t n_sites, const hyg_sg_chain* chains,
                                    const int32_t* chain_model, int32_t n_chains, double* log_z, double* final_lw,
                                    int32_t* final_st, int32_t* n_part, int32_t* status) {
  return sg_filter_host_impl(models, n_models, meth, tot, S, n_sites, chains, chain_model, n_chains, false, -1,
                             nullptr, nullptr, nullptr, log_z, final_lw, final_st, n_part, status);
}

int hyg_sg_trace_chains_host_multi(const hyg_sg_model* const* models, int32_t n_models, const uint16_t* meth,
                                   const uint16_t* tot, int32_t S, int64_t n_sites, const hyg_sg_chain* chains,
                                   const int32_t* chain_model, int32_t n_chains, int64_t out_rows, double* log_z_t,
                                   double* regime_probs, double* cp_probs, double* log_z, double* final_lw,
                                   int32_t* final_st, int32_t* n_part, int32_t* status) {
  return sg_filter_host_impl(models, n_models, meth, tot, S, n_sites, chains, chain_model, n_chains, true, out_rows,
                             log_z_t, regime_probs, cp_probs, log_z, final_lw, final_st, n_part, status);
}

// ---- joint segmentations by backward simulation (hyg_sg_history_chains_multi, hyg_sg_sample_paths_multi)

int hyg_sg_history_chains_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                                const int32_t* chain_model, int32_t n_chains, const double* E, void* workspace,
                                size_t workspace_bytes, const hyg_sg_history* history, double* log_z,
                                double* final_lw, int32_t* final_st, int32_t* n_part, int32_t* status, void* stream) {
  return sg_filter_impl(models, n_models, chains, chain_model, true, n_chains, E, workspace, workspace_bytes, false,
                        nullptr, log_z, final_lw, final_st, n_part, status, stream, true, history);
}

int hyg_sg_sample_paths_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                              const int32_t* chain_model, int32_t n_chains, const hyg_sg_history* history,
                              const int32_t* forward_status, int32_t n_trajectories, int16_t* paths,
                              int32_t* sample_status, void* stream) {
  return sg_sample_impl(models, n_models, chains, chain_model, n_chains, history, forward_status, n_trajectories,
                        paths, sample_status, stream);
}

int hyg_sg_sample_chains_host_multi(const hyg_sg_model* const* models, int32_t n_models, const uint16_t* meth,
                                    const uint16_t* tot, int32_t S, int64_t n_sites, const hyg_sg_chain* chains,
                                    const int32_t* chain_model, int32_t n_chains, int32_t n_trajectories,
                                    int64_t out_rows, int16_t* paths, double* log_z, int32_t* status) {
  return sg_sample_host_impl(models, n_models, meth, tot, S, n_sites, chains, chain_model, n_chains, n_trajectories,
                             out_rows, paths, log_z, status);
}

int32_t hyg_sg_filter_kernel_name(const hyg_sg_model* m, char* buf, int32_t len) {
  return sg_filter_name_impl(&m, 1, false, false, buf, len);
}
int32_t hyg_sg_filter_kernel_name_multi(const hyg_sg_model* const* models, int32_t n_models, char* buf, int32_t len) {
  return sg_filter_name_impl(models, n_models, true, false, buf, len);
}
int32_t hyg_sg_trace_kernel_name(const hyg_sg_model* m, char* buf, int32_t len) {
  return sg_filter_name_impl(&m, 1, false, true, buf, len);
}
int32_t hyg_sg_trace_kernel_name_multi(const hyg_sg_model* const* models, int32_t n_models, char* buf, int32_t len) {
  return sg_filter_name_impl(models, n_models, true, true, buf, len);
}

// ---- regime BED tracks

int hyg_bed_labels(const double* probs, int32_t K, int64_t n, int8_t* label, double* score, void* stream) {
  if (K < 1 || K > HYG_KMAX || n < 0) return fail(HYG_EINVAL, "K out of [1, 16] or negative n_sites");
  if (n > 0 && (!probs || !label || !score)) return fail(HYG_EINVAL, "null buffer");
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device: hygeia_amd has no CPU fallback");
  const int rc = bed_launch_labels(probs, K, n, label, score, stream);
  if (rc != HYG_OK) return fail(rc, "label launch failed");
  return HYG_OK;
}

int64_t hyg_bed_format(const char* chrom, const int64_t* pos, const int8_t* label, const double* score, int64_t n,
                       int32_t K, const char* const* names, const char* const* rgb, char* out, int64_t out_bytes) {
  if (!chrom || K < 1 || K > HYG_KMAX || n < 0 || !names || !rgb) return fail(HYG_EINVAL, "invalid argument");
  if (n > 0 && (!pos || !label || !score)) return fail(HYG_EINVAL, "null buffer");
  for (int r = 0; r <= K; ++r)
    if (!names[r] || !rgb[r]) return fail(HYG_EINVAL, "null name or colour");
  int64_t need = 0;
  char line[512];
  for (int64_t i = 0; i < n; ++i) {
    const int lb = label[i];
    if (lb < -1 || lb >= K) return fail(HYG_EINVAL, "label out of range");
    const int k = lb < 0 ? K : lb;
    char sc[64];
    // fwrite(scipen = 999): fixed notation, <= 15 significant digits, no trailing zeros
    int m = std::snprintf(sc, sizeof sc, "%.15g", score[i]);
    if (std::strchr(sc, 'e')) {  // tiny or huge values: positional form of the same digits
      m = std::snprintf(sc, sizeof sc, "%.17f", score[i]);
      while (m > 1 && sc[m - 1] == '0') sc[--m] = 0;
      if (m > 1 && sc[m - 1] == '.') sc[--m] = 0;
    }
    const long long a = (long long)pos[i] - 1, b = (long long)pos[i] + 1;
    const int len = std::snprintf(line, sizeof line, "%s\t%lld\t%lld\t%s\t%s\t.\t%lld\t%lld\t%s\n", chrom, a, b,
                                  names[k], sc, a, b, rgb[k]);
    if (len < 0 || len >= (int)sizeof line) return fail(HYG_EINVAL, "BED line too long");
    if (out && need + len <= out_bytes) std::memcpy(out + need, line, (size_t)len);
    need += len;
  }
  return need;
}

// ---- preprocess

int hyg_pre_collapse(const int64_t* pos0, int64_t T, const int64_t* plus_start, const int64_t* plus_end,
                     const double* plus_cov, const double* plus_pct, int64_t n_plus, const int64_t* minus_start,
                     const double* minus_cov, const double* minus_pct, int64_t n_minus, int32_t plus_single_base,
                     uint8_t* scratch, double* counts, int32_t stride, int32_t column, int32_t* conflicts,
                     void* stream) {
  if (T < 0 || n_plus < 0 || n_minus < 0 || stride < 2 || column < 0 || column + 2 > stride)
    return fail(HYG_EINVAL, "invalid sizes (need 0 <= column, column + 2 <= stride)");
  if ((T > 0 && (!pos0 || !counts || !conflicts)) || (n_plus > 0 && (!plus_start || !plus_end || !plus_cov || !plus_pct)) ||
      (n_minus > 0 && (!minus_start || !minus_cov || !minus_pct || (!scratch && !plus_single_base))))
    return fail(HYG_EINVAL, "null buffer");
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device: hygeia_amd has no CPU fallback");
  const int rc = pre_launch_collapse(pos0, T, plus_start, plus_end, plus_cov, plus_pct, n_plus, minus_start, minus_cov,
                                     minus_pct, n_minus, plus_single_base ? 1 : 0, scratch, counts, stride, column,
                                     conflicts, stream);
  if (rc != HYG_OK) return fail(rc, "preprocess launch failed");
  return HYG_OK;
}

}  // extern "C"

// ================================================ aggregation and DMPs
namespace {

// FDR_procedure's statistics in numpy's sorted order (ascending t = 1 - c/P,
// i.e. descending c), as runs of hist[c] equal values.
struct SortedStats {
  const std::vector<uint32_t>& hist;
  int P;
  double value(int c) const { return 1.0 - (double)c / (double)P; }
};

}  // namespace

extern "C" {

int hyg_tg_posterior_counts(const float* split, const float* regime, int32_t K, int32_t B, const int64_t* segments,
                            int32_t n_segments, int64_t max_rows, int32_t exclusive, int32_t* counts,
                            void* stream) {
  if (!split || !regime || !counts || (n_segments > 0 && !segments) || K < 1 || K > HYG_KMAX || B < 1 ||
      n_segments < 0 || max_rows < 0)
    return fail(HYG_EINVAL, "hyg_tg_posterior_counts: invalid arguments");
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device: hygeia_amd has no CPU fallback");
  if (launch_post_counts(split, regime, 2 * K, B, segments, n_segments, max_rows, exclusive != 0, counts, stream))
    return fail(HYG_EDEVICE, "posterior_counts launch failed");
  return HYG_OK;
}

int hyg_dmp_site_counts(const int16_t* merged, const int16_t* control, const int16_t* kase, int32_t B, int32_t K,
                        const hyg_dmp_group* groups, const int64_t* block_rows, int32_t n_groups, int32_t n_seeds,
                        int64_t n_sites, int32_t* counts, int32_t* pairs, void* stream) {
  if (!merged || !control || !kase || !counts || B < 1 || K < 1 || K > HYG_KMAX || n_groups < 0 || n_seeds < 1 ||
      (n_groups > 0 && (!groups || !block_rows)))
    return fail(HYG_EINVAL, "hyg_dmp_site_counts: invalid arguments");
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device");
  if (n_groups == 0) return HYG_OK;
  std::vector<int64_t> row0(n_groups + 1), site(n_groups);
  row0[0] = 0;
  for (int g = 0; g < n_groups; ++g) {
    if (groups[g].n_rows < 0 || groups[g].site_begin < 0 || groups[g].site_begin + groups[g].n_rows > n_sites)
      return fail(HYG_EINVAL, "hyg_dmp_site_counts: group outside [0, n_sites)");
    row0[g + 1] = row0[g] + groups[g].n_rows;
    site[g] = groups[g].site_begin;
  }
  DevBuf d_row0, d_site, d_blk;
  const size_t nb = (size_t)n_groups * n_seeds;
  if (!d_row0.alloc(sizeof(int64_t) * (n_groups + 1)) || !d_site.alloc(sizeof(int64_t) * n_groups) ||
      !d_blk.alloc(sizeof(int64_t) * nb))
    return fail(HYG_ENOMEM, "device allocation failed");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(d_row0.p, row0.data(), sizeof(int64_t) * (n_groups + 1), hipMemcpyHostToDevice, s) ||
      hipMemcpyAsync(d_site.p, site.data(), sizeof(int64_t) * n_groups, hipMemcpyHostToDevice, s) ||
      hipMemcpyAsync(d_blk.p, block_rows, sizeof(int64_t) * nb, hipMemcpyHostToDevice, s))
    return fail(HYG_EDEVICE, "copy failed");
  if (launch_dmp_site_counts(merged, control, kase, B, K, (const int64_t*)d_row0.p, (const int64_t*)d_site.p,
                             (const int64_t*)d_blk.p, n_groups, n_seeds, row0[n_groups], counts, pairs, stream))
    return fail(HYG_EDEVICE, "dmp_site_counts launch failed");
  // the descriptors are freed on return: wait for the kernel
  if (hipStreamSynchronize(s) != hipSuccess) return fail(HYG_EDEVICE, "kernel execution failed");
  return HYG_OK;
}

int hyg_dmp_fdr(const int32_t* counts, int32_t stride, int32_t column, int64_t n, int32_t P, double thr, int64_t* k,
                double* q_k, double* threshold, void* stream) {
  if (!counts || !k || !q_k || !threshold || n < 1 || P < 1 || stride < 1 || column < 0 || column >= stride)
    return fail(HYG_EINVAL, "hyg_dmp_fdr: invalid arguments");
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device");
  hipStream_t s = (hipStream_t)stream;
  DevBuf d_hist, d_bad;
  if (!d_hist.alloc(sizeof(uint32_t) * (P + 1)) || !d_bad.alloc(sizeof(int32_t)))
    return fail(HYG_ENOMEM, "device allocation failed");
  if (hipMemsetAsync(d_hist.p, 0, sizeof(uint32_t) * (P + 1), s) || hipMemsetAsync(d_bad.p, 0, 4, s))
    return fail(HYG_EDEVICE, "memset failed");
  if (launch_dmp_hist(counts, stride, column, n, P, (uint32_t*)d_hist.p, (int32_t*)d_bad.p, stream))
    return fail(HYG_EDEVICE, "dmp_hist launch failed");
  std::vector<uint32_t> hist(P + 1);
  int32_t bad = 0;
  if (hipMemcpyAsync(hist.data(), d_hist.p, sizeof(uint32_t) * (P + 1), hipMemcpyDeviceToHost, s) ||
      hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, s) || hipStreamSynchronize(s))
    return fail(HYG_EDEVICE, "kernel execution failed");
  if (bad) return fail(HYG_EINVAL, "hyg_dmp_fdr: a count lies outside [0, n_particles]");
  const SortedStats st{hist, P};
  int cmax = P;
  while (cmax >= 0 && hist[cmax] == 0) --cmax;
  // ordered_test_statistics[0] (:4) is the statistic of the largest count
  if (thr < st.value(cmax)) {  // (:8-9)
    *k = 0; *q_k = 0.0; *threshold = 0.0;
    return HYG_OK;
  }
  // Qs = 1./linspace(1, n, n) * cumsum(ordered) (:5-6), numpy's sequential
  // float64 cumsum; s = sum(Qs <= thr) (:7)
  double acc = 0.0, q_last = 0.0, q_s1 = 0.0;
  int64_t i = 0, cnt = 0;
  for (int c = cmax; c >= 0; --c) {
    const double v = st.value(c);
    for (uint32_t r = 0; r < hist[c]; ++r, ++i) {
      acc = (i == 0) ? v : acc + v;
      const double q = (1.0 / (double)(i + 1)) * acc;
      cnt += (q <= thr) ? 1 : 0;
      q_last = q;
    }
  }
  const int64_t sel = cnt;
  if (sel == n) {  // `s == test_statistics.shape` (:10-11)
    *k = n; *q_k = q_last; *threshold = 1.01;
    return HYG_OK;
  }
  // Qs[s-1] and ordered[s] (:12): replay up to position s
  acc = 0.0; i = 0;
  double ord_s = 0.0;
  bool done = false;
  for (int c = cmax; c >= 0 && !done; --c) {
    const double v = st.value(c);
    for (uint32_t r = 0; r < hist[c]; ++r, ++i) {
      if (i == sel) { ord_s = v; done = true; break; }
      acc = (i == 0) ? v : acc + v;
      q_s1 = (1.0 / (double)(i + 1)) * acc;
    }
  }
  *k = sel; *q_k = q_s1; *threshold = ord_s;
  return HYG_OK;
}

int hyg_dmp_weighted_fdr(const int32_t* counts, int32_t stride, int32_t column, int64_t n, int32_t P, double thr,
                         const double* w_fp, const double* w_fn, int64_t* ranked, int64_t* s_out, double* n_sum,
                         void* stream) {
  if (!counts || !w_fp || !w_fn || !ranked || !s_out || !n_sum || n < 1 || n > 0x7fffffffll || P < 1 ||
      stride < 1 || column < 0 || column >= stride)
    return fail(HYG_EINVAL, "hyg_dmp_weighted_fdr: invalid arguments");
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device");
  hipStream_t s = (hipStream_t)stream;
  DevBuf d_keys, d_vals, d_exc, d_tmp, d_er;
  if (!d_keys.alloc(8 * (size_t)n) || !d_vals.alloc(4 * (size_t)n) || !d_exc.alloc(8 * (size_t)n) ||
      !d_tmp.alloc(radix_temp_bytes(n)) || !d_er.alloc(8 * (size_t)n))
    return fail(HYG_ENOMEM, "device allocation failed");
  if (launch_dmp_rank(counts, stride, column, n, P, thr, w_fp, w_fn, (uint64_t*)d_keys.p, (uint32_t*)d_vals.p,
                      (double*)d_exc.p, stream))
    return fail(HYG_EDEVICE, "dmp_rank launch failed");
  if (radix_sort_pairs((uint64_t*)d_keys.p, (uint32_t*)d_vals.p, n, d_tmp.p, stream))
    return fail(HYG_EDEVICE, "radix sort launch failed");
  if (launch_dmp_gather((const uint32_t*)d_vals.p, (const double*)d_exc.p, n, (double*)d_er.p, ranked, stream))
    return fail(HYG_EDEVICE, "dmp_gather launch failed");
  std::vector<double> e((size_t)n);
  if (hipMemcpyAsync(e.data(), d_er.p, 8 * (size_t)n, hipMemcpyDeviceToHost, s) || hipStreamSynchronize(s))
    return fail(HYG_EDEVICE, "kernel execution failed");
  // Nsums = np.cumsum(ranked excess rates) (:20), s = sum(Nsums <= 0) (:21)
  double acc = 0.0;
  int64_t cnt = 0;
  for (int64_t i = 0; i < n; ++i) {
    acc = (i == 0) ? e[0] : acc + e[i];
    cnt += (acc <= 0.0) ? 1 : 0;
  }
  const int64_t last = (cnt == 0) ? n - 1 : cnt - 1;  // Nsums[s - 1]
  acc = 0.0;
  for (int64_t i = 0; i <= last; ++i) acc = (i == 0) ? e[0] : acc + e[i];
  *s_out = cnt;
  *n_sum = acc;
  return HYG_OK;
}

}  // extern "C"

// ============================================================= regions
extern "C" {

int hyg_dmr_find_regions(const int32_t* counts, int32_t stride, int32_t column, int64_t n_sites, int32_t min_count,
                         const int64_t* positions, int64_t max_gap, int32_t min_sites, int64_t* regions,
                         int64_t capacity, int64_t* n_regions, void* stream) {
  if (!n_regions) return fail(HYG_EINVAL, "hyg_dmr_find_regions: null n_regions");
  *n_regions = 0;
  if (!counts || !positions) return fail(HYG_EINVAL, "hyg_dmr_find_regions: null counts or positions");
  if (n_sites < 0 || n_sites > (1ll << 31)) return fail(HYG_EINVAL, "hyg_dmr_find_regions: n_sites outside [0, 2^31]");
  if (stride < 1 || column < 0 || column >= stride)
    return fail(HYG_EINVAL, "hyg_dmr_find_regions: column outside the stride");
  if (min_count < 0) return fail(HYG_EINVAL, "hyg_dmr_find_regions: min_count < 0");
  if (max_gap < 0) return fail(HYG_EINVAL, "hyg_dmr_find_regions: max_gap < 0");
  if (min_sites < 1) return fail(HYG_EINVAL, "hyg_dmr_find_regions: min_sites < 1");
  if (capacity < 0 || (capacity > 0 && !regions))
    return fail(HYG_EINVAL, "hyg_dmr_find_regions: null regions or negative capacity");
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device");
  if (n_sites == 0) return HYG_OK;
  hipStream_t s = (hipStream_t)stream;
  // pass 1: the runs of linked seed sites, counted, then written in order
  const int64_t nb = dmr_blocks(n_sites);
  DevBuf d_bs, d_tmp, d_tot, d_runs;
  if (!d_bs.alloc(sizeof(uint64_t) * (size_t)nb) || !d_tmp.alloc(dmr_scan_temp_bytes(nb)) || !d_tot.alloc(8))
    return fail(HYG_ENOMEM, "device allocation failed");
  if (launch_dmr_site_sums(counts, stride, column, n_sites, min_count, positions, max_gap, (uint64_t*)d_bs.p, d_tmp.p,
                           (uint64_t*)d_tot.p, stream))
    return fail(HYG_EDEVICE, "dmr_site_sums launch failed");
  uint64_t tot = 0;
  if (hipMemcpyAsync(&tot, d_tot.p, 8, hipMemcpyDeviceToHost, s) || hipStreamSynchronize(s))
    return fail(HYG_EDEVICE, "kernel execution failed");
  const int64_t n_runs = (int64_t)(tot >> 32);  // starts; the low half counts the ends
  if (n_runs != (int64_t)(tot & 0xffffffffull)) return fail(HYG_EDEVICE, "hyg_dmr_find_regions: starts != ends");
  if (n_runs == 0) return HYG_OK;
  if (!d_runs.alloc(sizeof(int64_t) * 2 * (size_t)n_runs)) return fail(HYG_ENOMEM, "device allocation failed");
  if (launch_dmr_site_emit(counts, stride, column, n_sites, min_count, positions, max_gap, (const uint64_t*)d_bs.p,
                           (int64_t*)d_runs.p, stream))
    return fail(HYG_EDEVICE, "dmr_site_emit launch failed");
  // pass 2: the runs of at least min_sites sites
  const int64_t nb2 = dmr_blocks(n_runs);
  DevBuf d_bs2, d_tmp2;
  if (!d_bs2.alloc(sizeof(uint64_t) * (size_t)nb2) || !d_tmp2.alloc(dmr_scan_temp_bytes(nb2)))
    return fail(HYG_ENOMEM, "device allocation failed");
  if (launch_dmr_run_sums((const int64_t*)d_runs.p, n_runs, min_sites, (uint64_t*)d_bs2.p, d_tmp2.p,
                          (uint64_t*)d_tot.p, stream))
    return fail(HYG_EDEVICE, "dmr_run_sums launch failed");
  if (hipMemcpyAsync(&tot, d_tot.p, 8, hipMemcpyDeviceToHost, s) || hipStreamSynchronize(s))
    return fail(HYG_EDEVICE, "kernel execution failed");
  *n_regions = (int64_t)tot;
  if (!regions) return HYG_OK;  // count only
  if ((int64_t)tot > capacity)
    return fail(HYG_EINVAL, "hyg_dmr_find_regions: " + std::to_string(tot) + " regions exceed the capacity " +
                                std::to_string(capacity));
  if (tot == 0) return HYG_OK;
  if (launch_dmr_run_emit((const int64_t*)d_runs.p, n_runs, min_sites, (const uint64_t*)d_bs2.p, regions, stream))
    return fail(HYG_EDEVICE, "dmr_run_emit launch failed");
  // the scratch is freed on return: wait for the kernel
  if (hipStreamSynchronize(s) != hipSuccess) return fail(HYG_EDEVICE, "kernel execution failed");
  return HYG_OK;
}

int hyg_dmr_region_counts(const int16_t* control, const int16_t* kase, int32_t B, const hyg_dmp_group* groups,
                          const int64_t* block_rows, int32_t n_groups, int32_t n_seeds, int64_t n_sites,
                          const int64_t* regions, int64_t n_regions, int32_t frac_num, int32_t frac_den,
                          int32_t* region_counts, void* stream) {
  if (!control || !kase) return fail(HYG_EINVAL, "hyg_dmr_region_counts: null trajectories");
  if (B < 1 || n_seeds < 1) return fail(HYG_EINVAL, "hyg_dmr_region_counts: B and n_seeds must be >= 1");
  if ((int64_t)B * n_seeds > kDmrMaxTrajectories)
    return fail(HYG_EINVAL, "hyg_dmr_region_counts: more than " + std::to_string(kDmrMaxTrajectories) +
                                " trajectories (B * n_seeds)");
  if (n_sites < 0 || n_regions < 0 || n_regions > 0x7fffffffll)
    return fail(HYG_EINVAL, "hyg_dmr_region_counts: n_sites or n_regions out of range");
  if (n_groups < 0 || (n_groups > 0 && (!groups || !block_rows)))
    return fail(HYG_EINVAL, "hyg_dmr_region_counts: null groups or block_rows");
  if (frac_den < 1 || frac_den > 1000 || frac_num < 0 || frac_num > frac_den)
    return fail(HYG_EINVAL, "hyg_dmr_region_counts: fraction must have 0 <= frac_num <= frac_den, 1 <= frac_den <= 1000");
  if (n_regions > 0 && (!regions || !region_counts))
    return fail(HYG_EINVAL, "hyg_dmr_region_counts: null regions or region_counts");
  int64_t prev_end = 0;
  for (int g = 0; g < n_groups; ++g) {
    if (groups[g].n_rows < 0 || groups[g].site_begin < 0 || groups[g].site_begin > n_sites ||
        groups[g].n_rows > n_sites - groups[g].site_begin)
      return fail(HYG_EINVAL, "hyg_dmr_region_counts: group " + std::to_string(g) + " outside [0, n_sites)");
    if (groups[g].site_begin < prev_end)
      return fail(HYG_EINVAL, "hyg_dmr_region_counts: groups must be sorted by site and disjoint (group " +
                                  std::to_string(g) + ")");
    prev_end = groups[g].site_begin + groups[g].n_rows;
    for (int sd = 0; sd < n_seeds; ++sd)
      if (block_rows[(size_t)g * n_seeds + sd] < 0)
        return fail(HYG_EINVAL, "hyg_dmr_region_counts: negative block row");
  }
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device");
  if (n_regions == 0) return HYG_OK;
  // descriptors: group begins, group ends, block rows
  const size_t nd = (size_t)n_groups * (2 + (size_t)n_seeds);
  std::vector<int64_t> desc(nd ? nd : 1, 0);
  for (int g = 0; g < n_groups; ++g) {
    desc[g] = groups[g].site_begin;
    desc[n_groups + g] = groups[g].site_begin + groups[g].n_rows;
  }
  for (size_t i = 0; i < (size_t)n_groups * n_seeds; ++i) desc[2 * (size_t)n_groups + i] = block_rows[i];
  DevBuf d_desc;
  if (!d_desc.alloc(sizeof(int64_t) * desc.size())) return fail(HYG_ENOMEM, "device allocation failed");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(d_desc.p, desc.data(), sizeof(int64_t) * desc.size(), hipMemcpyHostToDevice, s))
    return fail(HYG_EDEVICE, "copy failed");
  if (launch_dmr_region_counts(control, kase, B, (const int64_t*)d_desc.p, n_groups, n_seeds, n_sites, regions,
                               n_regions, frac_num, frac_den, region_counts, stream))
    return fail(HYG_EDEVICE, "dmr_region_counts launch failed");
  // the descriptors are freed on return: wait for the kernel
  if (hipStreamSynchronize(s) != hipSuccess) return fail(HYG_EDEVICE, "kernel execution failed");
  return HYG_OK;
}

int hyg_dmr_region_sums(const int32_t* counts, int32_t stride, int64_t n_sites, const int64_t* regions,
                        int64_t n_regions, int64_t* sums, void* stream) {
  if (!counts) return fail(HYG_EINVAL, "hyg_dmr_region_sums: null counts");
  if (stride < 1 || stride > kDmrMaxStride)
    return fail(HYG_EINVAL, "hyg_dmr_region_sums: stride outside [1, " + std::to_string(kDmrMaxStride) + "]");
  if (n_sites < 0 || n_regions < 0 || n_regions > 0x7fffffffll)
    return fail(HYG_EINVAL, "hyg_dmr_region_sums: n_sites or n_regions out of range");
  if (n_regions > 0 && (!regions || !sums)) return fail(HYG_EINVAL, "hyg_dmr_region_sums: null regions or sums");
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device");
  if (n_regions == 0) return HYG_OK;
  if (launch_dmr_region_sums(counts, stride, n_sites, regions, n_regions, sums, stream))
    return fail(HYG_EDEVICE, "dmr_region_sums launch failed");
  return HYG_OK;
}

}  // extern "C"

// ========================================================= change points
namespace {

// The checks that the three trajectory arguments share (hyg_dmr_region_counts' rules); "" when they hold.
std::string cp_check_groups(const char* entry, int32_t B, const hyg_dmp_group* groups, const int64_t* block_rows,
                            int32_t n_groups, int32_t n_seeds, int64_t n_sites) {
  const std::string e = std::string(entry) + ": ";
  if (B < 1 || n_seeds < 1) return e + "B and n_seeds must be >= 1";
  if ((int64_t)B * n_seeds > hyg::kCpMaxTrajectories)
    return e + "more than " + std::to_string(hyg::kCpMaxTrajectories) + " trajectories (B * n_seeds)";
  if (n_sites < 0 || n_sites > (1ll << 31)) return e + "n_sites outside [0, 2^31]";
  if (n_groups < 0 || (n_groups > 0 && (!groups || !block_rows))) return e + "null groups or block_rows";
  int64_t prev_end = 0;
  for (int g = 0; g < n_groups; ++g) {
    if (groups[g].n_rows < 0 || groups[g].site_begin < 0 || groups[g].site_begin > n_sites ||
        groups[g].n_rows > n_sites - groups[g].site_begin)
      return e + "group " + std::to_string(g) + " outside [0, n_sites)";
    if (groups[g].site_begin < prev_end)
      return e + "groups must be sorted by site and disjoint (group " + std::to_string(g) + ")";
    prev_end = groups[g].site_begin + groups[g].n_rows;
    for (int sd = 0; sd < n_seeds; ++sd)
      if (block_rows[(size_t)g * n_seeds + sd] < 0) return e + "negative block row";
  }
  return "";
}

// descriptors on the device: group begins, group ends, block rows
bool cp_upload_groups(DevBuf& d_desc, const hyg_dmp_group* groups, const int64_t* block_rows, int32_t n_groups,
                      int32_t n_seeds, hipStream_t s) {
  const size_t nd = (size_t)n_groups * (2 + (size_t)n_seeds);
  std::vector<int64_t> desc(nd ? nd : 1, 0);
  for (int g = 0; g < n_groups; ++g) {
    desc[g] = groups[g].site_begin;
    desc[n_groups + g] = groups[g].site_begin + groups[g].n_rows;
  }
  for (size_t i = 0; i < (size_t)n_groups * n_seeds; ++i) desc[2 * (size_t)n_groups + i] = block_rows[i];
  if (!d_desc.alloc(sizeof(int64_t) * desc.size())) return false;
  // pageable memory: the copy has left desc when the call returns
  return hipMemcpyAsync(d_desc.p, desc.data(), sizeof(int64_t) * desc.size(), hipMemcpyHostToDevice, s) == hipSuccess;
}

}  // namespace

extern "C" {

int hyg_cp_site_events(const int16_t* merged, const int16_t* control, const int16_t* kase, int32_t B,
                       const hyg_dmp_group* groups, const int64_t* block_rows, int32_t n_groups, int32_t n_seeds,
                       int64_t n_sites, int32_t* events, void* stream) {
  if (!control || !kase) return fail(HYG_EINVAL, "hyg_cp_site_events: null trajectories (control or kase)");
  if (!events) return fail(HYG_EINVAL, "hyg_cp_site_events: null events");
  const std::string bad = cp_check_groups("hyg_cp_site_events", B, groups, block_rows, n_groups, n_seeds, n_sites);
  if (!bad.empty()) return fail(HYG_EINVAL, bad);
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device");
  if (n_sites == 0 || n_groups == 0) return HYG_OK;
  hipStream_t s = (hipStream_t)stream;
  DevBuf d_desc;
  if (!cp_upload_groups(d_desc, groups, block_rows, n_groups, n_seeds, s))
    return fail(HYG_ENOMEM, "device allocation or copy failed");
  if (launch_cp_site_events(merged, control, kase, B, (const int64_t*)d_desc.p, n_groups, n_seeds, n_sites, events,
                            stream))
    return fail(HYG_EDEVICE, "cp_site_events launch failed");
  // the descriptors are freed on return: wait for the kernel
  if (hipStreamSynchronize(s) != hipSuccess) return fail(HYG_EDEVICE, "kernel execution failed");
  return HYG_OK;
}

int hyg_cp_window_counts(const int16_t* merged, const int16_t* control, const int16_t* kase, int32_t B,
                         const hyg_dmp_group* groups, const int64_t* block_rows, int32_t n_groups, int32_t n_seeds,
                         int64_t n_sites, int32_t kind, const int64_t* windows, int64_t n_windows, int32_t* counts,
                         void* stream) {
  if (kind < 0 || kind >= kCpKinds) return fail(HYG_EINVAL, "hyg_cp_window_counts: kind outside [0, 4]");
  if (kind >= 3 && !merged)
    return fail(HYG_EINVAL, "hyg_cp_window_counts: null merged with kind 3 (split) or 4 (merge)");
  if (kind < 3 && (!control || !kase))
    return fail(HYG_EINVAL, "hyg_cp_window_counts: null trajectories (control or kase)");
  if (n_windows < 0 || n_windows > 0x7fffffffll)
    return fail(HYG_EINVAL, "hyg_cp_window_counts: n_windows out of range");
  const std::string bad = cp_check_groups("hyg_cp_window_counts", B, groups, block_rows, n_groups, n_seeds, n_sites);
  if (!bad.empty()) return fail(HYG_EINVAL, bad);
  if (n_windows > 0 && (!windows || !counts)) return fail(HYG_EINVAL, "hyg_cp_window_counts: null windows or counts");
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device");
  if (n_windows == 0) return HYG_OK;
  hipStream_t s = (hipStream_t)stream;
  DevBuf d_desc;
  if (!cp_upload_groups(d_desc, groups, block_rows, n_groups, n_seeds, s))
    return fail(HYG_ENOMEM, "device allocation or copy failed");
  if (launch_cp_window_counts(merged, control, kase, B, (const int64_t*)d_desc.p, n_groups, n_seeds, n_sites, kind,
                              windows, n_windows, counts, stream))
    return fail(HYG_EDEVICE, "cp_window_counts launch failed");
  if (hipStreamSynchronize(s) != hipSuccess) return fail(HYG_EDEVICE, "kernel execution failed");
  return HYG_OK;
}

int hyg_cp_window_intervals(const int32_t* events, int32_t stride, int32_t column, int64_t n_sites,
                            const int64_t* windows, int64_t n_windows, int32_t level_num, int32_t level_den,
                            int64_t* out, void* stream) {
  if (!events) return fail(HYG_EINVAL, "hyg_cp_window_intervals: null events");
  if (stride < 1 || column < 0 || column >= stride)
    return fail(HYG_EINVAL, "hyg_cp_window_intervals: column outside the stride");
  if (n_sites < 0 || n_sites > (1ll << 31)) return fail(HYG_EINVAL, "hyg_cp_window_intervals: n_sites outside [0, 2^31]");
  if (n_windows < 0 || n_windows > 0x7fffffffll)
    return fail(HYG_EINVAL, "hyg_cp_window_intervals: n_windows out of range");
  if (level_den < 1 || level_den > 1000 || level_num < 1 || level_num > level_den)
    return fail(HYG_EINVAL, "hyg_cp_window_intervals: level must have 0 < level_num <= level_den <= 1000");
  if (n_windows > 0 && (!windows || !out)) return fail(HYG_EINVAL, "hyg_cp_window_intervals: null windows or out");
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device");
  if (n_windows == 0) return HYG_OK;
  if (launch_cp_window_intervals(events, stride, column, n_sites, windows, n_windows, level_num, level_den, out, stream))
    return fail(HYG_EDEVICE, "cp_window_intervals launch failed");
  return HYG_OK;
}

}  // extern "C"

// ================================================= transition statistics
extern "C" {

int hyg_tg_transition_stats(const int16_t* merged, const int16_t* control, const int16_t* kase, int32_t B,
                            const hyg_dmp_group* groups, const int64_t* block_rows, int32_t n_groups, int32_t n_seeds,
                            int64_t n_sites, int32_t minimum_duration, int32_t dcap, int64_t* stats, void* stream) {
  if (!merged || !control || !kase)
    return fail(HYG_EINVAL, "hyg_tg_transition_stats: null trajectories (merged, control or kase)");
  if (!stats) return fail(HYG_EINVAL, "hyg_tg_transition_stats: null stats");
  if (dcap < 1 || dcap > kEmMaxDcap)
    return fail(HYG_EINVAL, "hyg_tg_transition_stats: dcap outside [1, " + std::to_string(kEmMaxDcap) + "]");
  if (minimum_duration < 0) return fail(HYG_EINVAL, "hyg_tg_transition_stats: negative minimum_duration");
  const std::string bad =
      cp_check_groups("hyg_tg_transition_stats", B, groups, block_rows, n_groups, n_seeds, n_sites);
  if (!bad.empty()) return fail(HYG_EINVAL, bad);
  if (!have_device()) return fail(HYG_EDEVICE, "no HIP device");
  if (n_sites == 0 || n_groups == 0) return HYG_OK;
  hipStream_t s = (hipStream_t)stream;
  DevBuf d_desc;
  if (!cp_upload_groups(d_desc, groups, block_rows, n_groups, n_seeds, s))
    return fail(HYG_ENOMEM, "device allocation or copy failed");
  if (launch_em_transition_stats(merged, control, kase, B, (const int64_t*)d_desc.p, n_groups, n_seeds, n_sites,
                                 minimum_duration, dcap, stats, stream))
    return fail(HYG_EDEVICE, "em_transition_stats launch failed");
  // the descriptors are freed on return: wait for the kernel
  if (hipStreamSynchronize(s) != hipSuccess) return fail(HYG_EDEVICE, "kernel execution failed");
  return HYG_OK;
}

}  // extern "C"
