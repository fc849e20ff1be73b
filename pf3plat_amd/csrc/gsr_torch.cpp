// gsr_torch.cpp - the torch-facing binding of the raster library: ONE translation unit, compiled against torch's headers by
// __graft_entry__.build() (pf3plat_amd/_lib.py::build_torch_ext) into pf3plat_amd/_gsr_torch.so.
//
// What it replaces: the reference's binding of its rasterizer is a compiled autograd function (the pybind module
// `diff_gaussian_rasterization._C` behind `_RasterizeGaussians`, imported at /root/reference/src/model/decoder/cuda_splatting.py:5-8 and
// called at :113-124).  Rounds 1-4 drove the C ABI (include/gsr.h) from a Python `torch.autograd.Function` through ctypes; per
// training step that layer cost more host time than the kernels take.  Here the same call contract lives in C++:
//   * the stream is torch's current HIP stream of the tensors' device (c10::hip::getCurrentHIPStream), the device is guarded;
//   * workspaces are ONE torch.uint8 allocation per call (three 2 MiB-aligned slices), kept in the autograd context for the backward;
//   * the pair-count policy (blocking status read + one retry | deferred verification at the end of the backward | lazy) is
//     HipBackend's of pf3plat_amd/rasterizer.py, moved here with its state (capacity hints, pending status copies);
//   * `RasterizeFn` is a torch::autograd::Function: no Python frame between torch's engine and gsr_backward;
//   * the plan API of HipBackend takes its workspaces, sizes and status reads from `Backend` too, and the small ops (camera set-up and
//     its backward, markVisible, covariances from scales / rotations) are here: only the plan API's launch calls use ctypes.
// The library itself is reached through dlopen + dlsym of the C ABI's entry points (the same file pf3plat_amd/_lib.py loads): nothing
// of torch crosses that boundary, only raw device pointers and the stream handle.  No CPU path: tensors must be on a ROCm device.
#include <torch/extension.h>
#include <torch/csrc/autograd/custom_function.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <sstream>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/gsr.h"

namespace {

using at::Tensor;

// ---- the C ABI, resolved at init() ------------------------------------------------------------------------------------------
struct Abi {
  void* handle = nullptr;
  decltype(&gsr_abi_version) abi_version = nullptr;
  decltype(&gsr_workspace_sizes) workspace_sizes = nullptr;
  decltype(&gsr_capacity_for) capacity_for = nullptr;
  decltype(&gsr_forward_ex) forward_ex = nullptr;
  decltype(&gsr_backward_ex) backward_ex = nullptr;
  decltype(&gsr_pose_partials_bytes) pose_partials_bytes = nullptr;
  decltype(&gsr_backward_scratch_bytes) backward_scratch_bytes = nullptr;
  decltype(&gsr_last_failed_stage) last_failed_stage = nullptr;
  decltype(&gsr_stage_name) stage_name = nullptr;
  decltype(&gsr_pack_view) pack_view = nullptr;
  decltype(&gsr_setup_views) setup_views = nullptr;
  decltype(&gsr_setup_views_backward) setup_views_backward = nullptr;
  decltype(&gsr_setup_views_backward_ex) setup_views_backward_ex = nullptr;
  decltype(&gsr_setup_views_orthographic) setup_views_orthographic = nullptr;
  decltype(&gsr_mark_visible) mark_visible = nullptr;
  decltype(&gsr_cov_from_scale_rot) cov_from_scale_rot = nullptr;
  decltype(&gsr_cov_from_scale_rot_backward) cov_from_scale_rot_backward = nullptr;
  decltype(&gsr_adapt) adapt = nullptr;
  decltype(&gsr_adapt_backward_ex) adapt_backward_ex = nullptr;
  decltype(&gsr_adapt_partials_bytes_ex) adapt_partials_bytes_ex = nullptr;
} g_abi;

template <class F>
void resolve(F& f, const char* name) {
  f = reinterpret_cast<F>(dlsym(g_abi.handle, name));
  TORCH_CHECK(f != nullptr, "pf3plat_amd: symbol ", name, " is missing from the raster library");
}

void init(const std::string& path) {
  if (g_abi.handle != nullptr) return;
  g_abi.handle = dlopen(path.c_str(), RTLD_NOW | RTLD_GLOBAL);
  TORCH_CHECK(g_abi.handle != nullptr, "pf3plat_amd: cannot load ", path, " (", dlerror(), "): the MI355X rasterizer has no fallback path");
  resolve(g_abi.abi_version, "gsr_abi_version");
  resolve(g_abi.workspace_sizes, "gsr_workspace_sizes");
  resolve(g_abi.capacity_for, "gsr_capacity_for");
  resolve(g_abi.forward_ex, "gsr_forward_ex");
  resolve(g_abi.backward_ex, "gsr_backward_ex");
  resolve(g_abi.pose_partials_bytes, "gsr_pose_partials_bytes");
  resolve(g_abi.backward_scratch_bytes, "gsr_backward_scratch_bytes");
  resolve(g_abi.last_failed_stage, "gsr_last_failed_stage");
  resolve(g_abi.stage_name, "gsr_stage_name");
  resolve(g_abi.pack_view, "gsr_pack_view");
  resolve(g_abi.setup_views, "gsr_setup_views");
  resolve(g_abi.setup_views_backward, "gsr_setup_views_backward");
  resolve(g_abi.setup_views_backward_ex, "gsr_setup_views_backward_ex");
  resolve(g_abi.setup_views_orthographic, "gsr_setup_views_orthographic");
  resolve(g_abi.mark_visible, "gsr_mark_visible");
  resolve(g_abi.cov_from_scale_rot, "gsr_cov_from_scale_rot");
  resolve(g_abi.cov_from_scale_rot_backward, "gsr_cov_from_scale_rot_backward");
  resolve(g_abi.adapt, "gsr_adapt");
  resolve(g_abi.adapt_backward_ex, "gsr_adapt_backward_ex");
  resolve(g_abi.adapt_partials_bytes_ex, "gsr_adapt_partials_bytes_ex");
  TORCH_CHECK(g_abi.abi_version() == GSR_ABI_VERSION, "pf3plat_amd: raster library ABI ", g_abi.abi_version(), " != ", GSR_ABI_VERSION, "; rebuild");
}

// ---- small helpers ----------------------------------------------------------------------------------------------------------
constexpr int kViewFloats = 48;  // sizeof(GsrView) / 4

void check_device(std::initializer_list<const Tensor*> ts) {
  for (const Tensor* t : ts)
    TORCH_CHECK(!t->defined() || t->is_cuda(), "pf3plat_amd rasterizer: tensors must be on a ROCm device (there is no CPU fallback path)");
}
Tensor f32c(const Tensor& t) {  // fp32 + contiguous, touching nothing when the tensor already is
  if (!t.defined() || (t.scalar_type() == at::kFloat && t.is_contiguous())) return t;
  return t.to(at::kFloat).contiguous();
}
const float* fptr(const Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }
float* fptr_mut(Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }
hipStream_t stream_of(const at::Device& d) { return c10::hip::getCurrentHIPStream(d.index()).stream(); }

void rc_check(int rc, const char* what, bool backward) {
  if (rc == 0) return;
  std::string msg = std::string(what) + " failed with code " + std::to_string(rc);
  if (rc == GSR_ERR_LAUNCH) {
    const char* stage = g_abi.stage_name(backward, g_abi.last_failed_stage());
    if (stage) msg += std::string(" (debug mode: stage '") + stage + "' did not complete)";
  }
  throw std::runtime_error(msg);
}

// The call shape (pf3plat_amd.rasterizer.RasterConfig, field for field: kCfgFields below is the one statement of names and order)
struct Cfg {
  int num_views = 0, num_sets = 0, views_per_set = 0, num_gaussians = 0, height = 0, width = 0, sh_degree = 0, sh_coeffs = 0, max_sh_eval = 4;
  int has_extra = 0, flags = 0, scale_rot = 0;
  int alpha = 0;  // the accumulated-alpha image is wanted (GsrForwardOptions.out_alpha / GsrBackwardOptions.dL_dalpha_img); not part of the dims: it sizes nothing
  // the dims of the sizing helpers: without the GSR_FLAG_SH_IN_FRAME bits, which only the launches take (they size nothing)
  GsrDims dims(int64_t capacity) const { GsrDims d = launch_dims(capacity); d.flags &= ~kShFrameBits; return d; }
  GsrDims launch_dims(int64_t capacity) const {
    GsrDims d;
    d.abi_version = GSR_ABI_VERSION; d.num_views = num_views; d.num_sets = num_sets; d.views_per_set = views_per_set;
    d.num_gaussians = num_gaussians; d.height = height; d.width = width; d.sh_degree = sh_degree; d.sh_coeffs = sh_coeffs;
    d.max_sh_eval = max_sh_eval; d.has_extra = has_extra; d.flags = flags; d.pair_capacity = capacity;
    return d;
  }
  static constexpr int kShFrameBits = GSR_FLAG_SH_IN_FRAME | GSR_FLAG_SH_FRAME_E3NN;
  int extra_mode() const { return (flags >> 4) & 7; }
};
// Cfg's fields, in the dataclass's order (exported as CFG_FIELDS): what crosses to and from Python by name, and what orders two call shapes
struct CfgField { const char* name; int Cfg::*member; bool is_bool; };
constexpr CfgField kCfgFields[] = {
    {"num_views", &Cfg::num_views, false}, {"num_sets", &Cfg::num_sets, false}, {"views_per_set", &Cfg::views_per_set, false}, {"num_gaussians", &Cfg::num_gaussians, false},
    {"height", &Cfg::height, false}, {"width", &Cfg::width, false}, {"sh_degree", &Cfg::sh_degree, false}, {"sh_coeffs", &Cfg::sh_coeffs, false},
    {"max_sh_eval", &Cfg::max_sh_eval, false}, {"has_extra", &Cfg::has_extra, true}, {"flags", &Cfg::flags, false}, {"scale_rot", &Cfg::scale_rot, true}, {"alpha", &Cfg::alpha, true}};
bool operator<(const Cfg& a, const Cfg& b) {
  for (const CfgField& f : kCfgFields) if (a.*f.member != b.*f.member) return a.*f.member < b.*f.member;
  return false;
}
}  // namespace
// How the two structs cross the binding: the call shape as any object with RasterConfig's attributes (-> a RasterConfig), the dims as any
// buffer of sizeof(GsrDims) bytes, which the ctypes mirror pf3plat_amd._lib.GsrDims is (-> one of those).  Anything else is a TypeError.
namespace pybind11::detail {
template <> struct type_caster<Cfg> {
  PYBIND11_TYPE_CASTER(Cfg, const_name("RasterConfig"));
  bool load(handle src, bool) {
    for (const CfgField& f : kCfgFields) {
      if (!hasattr(src, f.name)) return false;
      const object a = getattr(src, f.name);
      make_caster<int> as_int;  // (refuses floats; a bool field takes a bool or an integer, as RasterConfig's callers write them)
      if (f.is_bool ? !PyLong_Check(a.ptr()) : !as_int.load(a, true)) return false;
      value.*f.member = f.is_bool ? PyObject_IsTrue(a.ptr()) : (int)as_int;
    }
    return true;
  }
  static handle cast(const Cfg& c, return_value_policy, handle) {
    dict kw;
    for (const CfgField& f : kCfgFields) kw[f.name] = f.is_bool ? object(bool_(c.*f.member != 0)) : object(int_(c.*f.member));
    return module_::import("pf3plat_amd.rasterizer").attr("RasterConfig")(**kw).release();
  }
};
template <> struct type_caster<GsrDims> {
  PYBIND11_TYPE_CASTER(GsrDims, const_name("GsrDims"));
  bool load(handle src, bool) {
    Py_buffer view;
    if (!PyObject_CheckBuffer(src.ptr()) || PyObject_GetBuffer(src.ptr(), &view, PyBUF_SIMPLE) != 0) { PyErr_Clear(); return false; }
    const bool fits = view.len == (Py_ssize_t)sizeof(GsrDims);
    if (fits) std::memcpy(&value, view.buf, sizeof(GsrDims));
    PyBuffer_Release(&view);
    return fits;
  }
  static handle cast(const GsrDims& d, return_value_policy, handle) {
    return module_::import("pf3plat_amd._lib").attr("GsrDims").attr("from_buffer_copy")(bytes(reinterpret_cast<const char*>(&d), sizeof d)).release();
  }
};
}  // namespace pybind11::detail
namespace {
// The per-group rotations of the scale / rotation form: (sets, F, 3, 3) fp32 contiguous, or undefined
Tensor frames_arg(const Cfg& cfg, const Tensor& frames) {
  if (!frames.defined()) return frames;
  if (frames.dim() != 4 || frames.size(0) != cfg.num_sets || frames.size(2) != 3 || frames.size(3) != 3 || frames.size(1) == 0 ||
      cfg.num_gaussians % frames.size(1))
    throw pybind11::value_error("frames must be (sets, F, 3, 3) with F dividing the number of Gaussians");
  return frames.detach().to(at::kFloat).contiguous();  // (a QR factor, e.g., arrives column-major)
}
// The options of an _ex launch from the call shape, its checked frames (`fr`: frames_arg's result) and its alpha image - the forward's
// output, the backward's cotangent; undefined: a NULL field, the launch without alpha.  Both tensors stay alive until the call returns.
template <class Options>
Options launch_options(const Cfg& cfg, const Tensor& fr, const Tensor& alpha) {
  Options opt{};
  opt.frames = fptr(fr); opt.num_frames = fr.defined() ? (int)fr.size(1) : 0; opt.scale_rot = cfg.scale_rot;
  float* const a = alpha.defined() ? alpha.data_ptr<float>() : nullptr;
  if constexpr (std::is_same_v<Options, GsrForwardOptions>) opt.out_alpha = a;
  else opt.dL_dalpha_img = a;
  return opt;
}

struct Status {
  int64_t num_pairs = 0;
  int overflow = 0, max_list = 0;
};

// A 16-byte pinned buffer the status block is copied into behind the forward.  The host writes a sentinel first: the copy has landed
// when the sentinel is gone (num_pairs and max_list are never negative).  No event object, no blocking call on the usual path - a
// blocking copy / synchronize sleeps and wakes up 30-60 us late.
struct Pinned {
  volatile int64_t* q = nullptr;  // [0]: num_pairs; as int32: [2] overflow, [3] max_list
  volatile int32_t* w() const { return reinterpret_cast<volatile int32_t*>(q); }
  void arm() { q[0] = -1; w()[3] = -1; }
  bool arrived() const { return q[0] != -1 && w()[3] != -1; }
};

using ShapeKey = std::tuple<int, int, int, int>;  // (views, N, H, W)

struct PendingItem {
  Pinned host;
  ShapeKey key;
  Cfg cfg;
  int64_t token;
  bool raises;
  int device;
};

struct Saved {  // what a differentiated forward hands its backward
  bool valid = false;
  GsrDims dims;
  Tensor geom, bin, img;
  int64_t token = 0;
};

struct ForwardOut {
  Tensor color, extra_img, radii;
  Saved saved;
  Tensor alpha_img;  // (V, H, W), only when the call shape asks for it (Cfg::alpha)
};

struct Plan {
  GsrDims dims;
  Tensor color, extra_img, radii, geom, bin, img;
  Tensor alpha_img;
};

struct Sizes { size_t geom = 0, bin = 0, img = 0, scratch = 0; };

class Backend : public std::enable_shared_from_this<Backend> {
 public:
  // policy (see pf3plat_amd/rasterizer.py::HipBackend for the full statement).  Atomics: Python sets them while a
  // forward runs without the GIL and a backward runs on one of the autograd engine's threads.
  enum class SyncPolicy { sync, lazy };
  enum class OnOverflow { raise, nan };  // nan: opted into by callers whose loop skips NaN-gradient steps (DecoderSplattingCUDA does)
  std::atomic<SyncPolicy> sync_policy{SyncPolicy::sync};
  std::atomic<int> defer_after{4};
  std::atomic<OnOverflow> on_overflow{OnOverflow::raise};
  std::atomic<bool> defer_status{false};
  std::atomic<double> spin_us{300.0};
  // head-room of a workspace sized from a shape's history: running maximum x clamp(1 + headroom_sigmas x sigma / mean, headroom_min, headroom_max)
  // of the pair counts seen for the shape (a new scene every step: tools/skip_rate.py -> profiles/r06_skip_rate.md)
  std::atomic<double> headroom_min{1.25}, headroom_max{3.0}, headroom_sigmas{4.0};

  ~Backend() {
    for (Pinned& p : pool_) (void)hipHostFree((void*)p.q);
    for (PendingItem& it : pending_) (void)hipHostFree((void*)it.host.q);
  }

  // ---- state the tests and the tools look at
  std::map<ShapeKey, int64_t> capacity_hint() { std::lock_guard<std::mutex> g(mu_); return hint_; }
  std::map<ShapeKey, int64_t> seen() { std::lock_guard<std::mutex> g(mu_); return seen_; }
  std::vector<int64_t> pending_tokens() { std::lock_guard<std::mutex> g(mu_); std::vector<int64_t> t; for (auto& p : pending_) t.push_back(p.token); return t; }
  std::vector<int64_t> poisoned_tokens() { std::lock_guard<std::mutex> g(mu_); return std::vector<int64_t>(poisoned_.begin(), poisoned_.end()); }
  bool has_status() { std::lock_guard<std::mutex> g(mu_); return has_status_; }
  bool any_pending() { std::lock_guard<std::mutex> g(mu_); return !pending_.empty(); }
  Status last_status() { std::lock_guard<std::mutex> g(mu_); return last_; }
  void set_capacity_hint(const ShapeKey& k, int64_t v) { std::lock_guard<std::mutex> g(mu_); hint_[k] = v; }
  // the head-room factor the next deferred / lazy call of this shape is sized with (1.25 until two status blocks have been read)
  double headroom_for(const ShapeKey& k) {
    std::lock_guard<std::mutex> g(mu_);
    auto it = stats_.find(k);
    return it == stats_.end() ? headroom_min.load() : factor_of(it->second);
  }

  int64_t capacity_for(const Cfg& cfg, const Status& st, double headroom = 1.25) const {
    const GsrDims d = cfg.dims(0);
    const int64_t need = g_abi.capacity_for(&d, (uint64_t)((double)st.num_pairs * headroom) + 4096u, (uint32_t)((double)st.max_list * headroom) + 16u);
    TORCH_CHECK(need >= 0, "gsr_capacity_for failed with code ", need);
    return need;
  }

  // The plan API's read-back: the status block at the head of `bin`, copied behind the work on the current stream and waited for.  It
  // feeds none of the policy's state (hints, statistics, `seen`, `last_status`).
  Status read_status(const Tensor& bin) {
    check_device({&bin});
    TORCH_CHECK(bin.nbytes() >= 16, "read_status: the bin workspace holds no status block");
    const at::Device dev = bin.device();
    c10::hip::HIPGuard guard(dev.index());
    const Pinned host = status_copy(bin, stream_of(dev));
    wait_status(host, dev.index());
    return take_status(host);
  }

  void release_workspaces() {
    if (any_pending()) check_pending(true, -1);
    std::lock_guard<std::mutex> g(mu_);
    ws_cache_.clear();
    sizes_.clear();
  }
  size_t workspace_cache_size() { std::lock_guard<std::mutex> g(mu_); return ws_cache_.size(); }

  // ---- the autograd-facing forward: fresh outputs per call; fresh workspaces too (kept for the backward) unless the caller says that
  // nothing will be differentiated (reuse_workspaces)
  ForwardOut forward(const Cfg& cfg, const Tensor& viewbuf, const Tensor& means, const Tensor& cov, const Tensor& opac, const Tensor& colors,
                     const Tensor& extra, const Tensor& frames, int64_t capacity /* <= 0: policy */, bool reuse_workspaces, bool one_view = false) {
    check_device({&viewbuf, &means, &cov, &opac, &colors, &extra, &frames});
    if (any_pending()) check_pending(false, -1);
    const at::Device dev = viewbuf.device();
    const ShapeKey key{cfg.num_views, cfg.num_gaussians, cfg.height, cfg.width};
    c10::hip::HIPGuard guard(dev.index());
    const hipStream_t stream = stream_of(dev);
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cap_status);
    bool known;
    {
      std::lock_guard<std::mutex> g(mu_);
      known = capacity <= 0 && hint_.count(key) != 0;
    }
    if (cap_status != hipStreamCaptureStatusNone) {  // nothing can be read back while a graph is being captured: the caller sizes
      TORCH_CHECK(capacity > 0 || known, "gsr_forward under stream capture: pass `capacity` (or run the shape once outside the capture)");
      Plan plan = make_plan(cfg, dev, capacity > 0 ? capacity : default_capacity(cfg), false, one_view);
      run_forward(plan, cfg, viewbuf, means, cov, opac, colors, extra, frames, stream);
      ForwardOut o{plan.color, plan.extra_img, plan.radii, {}, plan.alpha_img};
      o.saved = Saved{true, plan.dims, plan.geom, plan.bin, plan.img, 0};
      return o;
    }
    const bool lazy_policy = sync_policy == SyncPolicy::lazy, defer_all = defer_status;  // (each knob read once per call)
    const int after = defer_after;
    bool lazy = (lazy_policy && known) || defer_all;
    if (!lazy && known && !reuse_workspaces && (cfg.flags & GSR_FLAG_BACKWARD_FOLLOWS) && after > 0) {
      std::lock_guard<std::mutex> g(mu_);
      auto it = seen_.find(key);
      if (it != seen_.end() && it->second >= after) lazy = true;
    }
    int64_t cap = capacity > 0 ? capacity : default_capacity(cfg);
    for (int attempt = 0; attempt < 3; ++attempt) {
      Plan plan = make_plan(cfg, dev, cap, reuse_workspaces && !lazy, one_view);
      run_forward(plan, cfg, viewbuf, means, cov, opac, colors, extra, frames, stream);
      int64_t token;
      {
        std::lock_guard<std::mutex> g(mu_);
        token = ++token_;
      }
      ForwardOut out{plan.color, plan.extra_img, plan.radii, {}, plan.alpha_img};
      if (!reuse_workspaces) out.saved = Saved{true, plan.dims, plan.geom, plan.bin, plan.img, token};
      if (cfg.num_gaussians == 0 || cfg.num_views == 0) return out;
      if (lazy) {
        // (the 16 bytes are copied behind the forward on its stream; the caching allocator hands freed memory to later work of that
        // stream only, so nothing here needs to keep the workspace alive)
        PendingItem it{status_copy(plan.bin, stream), key, cfg, token, lazy_policy || defer_all || on_overflow == OnOverflow::raise, (int)dev.index()};
        std::lock_guard<std::mutex> g(mu_);
        pending_.push_back(it);
        return out;
      }
      Pinned host = status_copy(plan.bin, stream);
      wait_status(host, dev.index());
      const Status st = take_status(host);
      note_status(key, cfg, st);
      if (!st.overflow) return out;
      cap = capacity_for(cfg, st, 1.05);
    }
    throw std::runtime_error("gsr_forward: pair workspace overflowed repeatedly");
  }

  // Verify the status blocks of earlier lazy / deferred forwards (those whose copy has landed; all if `wait`; only_token >= 0: just
  // that forward, waiting for it).
  void check_pending(bool wait, int64_t only_token) {
    std::vector<PendingItem> items;
    {
      std::lock_guard<std::mutex> g(mu_);
      items.swap(pending_);
    }
    std::vector<PendingItem> keep;
    int64_t failed = -1, warned = -1;
    for (size_t k = 0; k < items.size(); ++k) {
      PendingItem& it = items[k];
      const bool mine = only_token >= 0 && it.token == only_token;
      if (only_token >= 0 && !mine) { keep.push_back(it); continue; }
      if (wait || mine) {
        try {
          wait_status(it.host, it.device);
        } catch (...) {  // (a device error while waiting: nothing is dropped - this item and the ones behind it stay pending)
          keep.insert(keep.end(), items.begin() + k, items.end());
          std::lock_guard<std::mutex> g(mu_);
          pending_.insert(pending_.begin(), keep.begin(), keep.end());
          throw;
        }
      } else if (!it.host.arrived()) { keep.push_back(it); continue; }
      const Status st = take_status(it.host);
      note_status(it.key, it.cfg, st);
      if (st.overflow) {
        if (it.raises) { if (failed < 0) failed = st.num_pairs; }
        else {
          warned = st.num_pairs;
          std::lock_guard<std::mutex> g(mu_);
          poisoned_.insert(it.token);
          while (poisoned_.size() > 4096) poisoned_.erase(poisoned_.begin());
        }
      }
    }
    if (!keep.empty()) {
      std::lock_guard<std::mutex> g(mu_);
      pending_.insert(pending_.begin(), keep.begin(), keep.end());
    }
    if (warned >= 0) {
      const std::string msg = "pf3plat_amd rasterizer: a training forward needed " + std::to_string(warned) +
                              " (tile, Gaussian) pairs, more than the head-room over the largest count seen for its shape: its image is NaN and its backward "
                              "returns NaN gradients (the step is skipped by a NaN-gradient guard such as the reference's); the workspace has "
                              "been enlarged for the next step.";
      pybind11::gil_scoped_acquire gil;  // (the backward runs on one of the engine's threads)
      // pf3plat_amd._lib.RasterOverflowWarning: a RuntimeWarning registered with the "always" filter - EVERY skipped step is reported,
      // not the first one per code location
      pybind11::object cls = pybind11::module_::import("pf3plat_amd._lib").attr("RasterOverflowWarning");
      if (PyErr_WarnEx(cls.ptr(), msg.c_str(), 1) < 0) throw pybind11::error_already_set();
    }
    if (failed >= 0)
      throw std::runtime_error("an earlier gsr_forward needed " + std::to_string(failed) +
                               " pairs but its workspace was smaller; that call's image was poisoned with NaN. The capacity hint has been raised - "
                               "re-run the step (or use sync_policy='sync' with defer_after = 0).");
  }

  // -> true when that forward overflowed and the policy is to answer with NaN gradients instead of raising.  The token STAYS in the
  // set: every backward over that forward (retain_graph, several autograd.grad calls) gets the same answer - numbers computed from an
  // overflowed forward's workspace are meaningless.  (Tokens only grow; the set keeps the newest 4096.)
  bool verify_own_forward(int64_t token) {
    if (any_pending()) check_pending(false, token);
    std::lock_guard<std::mutex> g(mu_);
    return poisoned_.count(token) != 0;
  }

  // -> d_means, d_cov, d_opac, d_colors, d_extra, d_means2d, d_views (undefined where not asked for)
  std::vector<Tensor> backward(const Cfg& cfg, const Saved& saved, const Tensor& viewbuf, const Tensor& means, const Tensor& cov, const Tensor& opac,
                               const Tensor& colors, const Tensor& extra_in, const Tensor& g_color_in, const Tensor& g_extra_in, bool want_means2d,
                               bool rows_in_workspace, const Tensor& frames, int want_views /* 0 none, 1 all, 2 depth term */,
                               const Tensor& g_alpha_in = Tensor() /* dL/d accumulated alpha (V, H, W); undefined: none */) {
    TORCH_CHECK(saved.valid, "this forward ran with reuse_workspaces=True (nothing was to be differentiated): it has no backward");
    const at::Device dev = viewbuf.device();
    c10::hip::HIPGuard guard(dev.index());
    const hipStream_t stream = stream_of(dev);
    const int v = cfg.num_views, n = cfg.num_gaussians, s = cfg.num_sets;
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    const bool own_rows = rows_in_workspace && (cfg.flags & GSR_FLAG_BACKWARD_FOLLOWS);
    Tensor scratch;
    if (!own_rows) scratch = at::empty({(int64_t)std::max<size_t>(16, sized(cfg, saved.dims.pair_capacity).scratch)}, f32.dtype(at::kByte));
    Tensor d_means = at::empty({s, n, 3}, f32);
    Tensor d_cov = cfg.scale_rot ? at::empty({s, n, 7}, f32) : (cfg.flags & GSR_FLAG_COV_3X3) ? at::empty({s, n, 3, 3}, f32) : at::empty({s, n, 6}, f32);
    Tensor d_opac = at::empty({s, n}, f32);
    Tensor d_colors = at::empty_like(colors);
    Tensor d_extra = (cfg.has_extra && !cfg.extra_mode()) ? at::empty({v, n}, f32) : Tensor();
    Tensor d_means2d = want_means2d ? at::empty({v, n, 3}, f32) : Tensor();
    Tensor d_views;
    const Tensor extra = (cfg.has_extra && !cfg.extra_mode()) ? extra_in : Tensor();
    if (n > 0 && v > 0) {
      const Tensor g_color = f32c(g_color_in);
      Tensor g_extra;
      if (cfg.has_extra) g_extra = g_extra_in.defined() ? f32c(g_extra_in) : at::zeros({v, cfg.height, cfg.width}, f32);
      if (want_views) d_views = at::empty({v, kViewFloats}, f32);
      const GsrView* vb = reinterpret_cast<const GsrView*>(viewbuf.data_ptr<float>());
      const Tensor fr = cfg.scale_rot ? frames_arg(cfg, frames) : Tensor();
      const Tensor g_alpha = f32c(g_alpha_in);
      if (g_alpha.defined()) TORCH_CHECK(g_alpha.numel() == (int64_t)v * cfg.height * cfg.width, "dL/dalpha must be (views, H, W)");
      GsrBackwardOptions opt = launch_options<GsrBackwardOptions>(cfg, fr, g_alpha);
      Tensor partials;
      if (want_views) {
        // (the helpers take no GSR_FLAG_SH_IN_FRAME bits; they change no size.  GSR_FLAG_FOV_GRADIENT stays: it widens the rows)
        GsrDims sizing_dims = saved.dims;
        sizing_dims.flags &= ~Cfg::kShFrameBits;
        partials = at::empty({(int64_t)std::max<size_t>(16, g_abi.pose_partials_bytes(&sizing_dims))}, f32.dtype(at::kByte));
        opt.dL_dviews = d_views.data_ptr<float>(); opt.pose_partials = reinterpret_cast<float*>(partials.data_ptr()); opt.depth_term_only = want_views == 2;
      }
      void* const scr = scratch.defined() ? scratch.data_ptr() : nullptr;
      const int rc = g_abi.backward_ex(&saved.dims, vb, fptr(means), fptr(cov), fptr(opac), fptr(colors), fptr(extra), saved.geom.data_ptr(), saved.bin.data_ptr(),
                                       saved.img.data_ptr(), fptr(g_color), fptr(g_extra), scr, fptr_mut(d_means), fptr_mut(d_cov), fptr_mut(d_opac),
                                       fptr_mut(d_colors), fptr_mut(d_extra), fptr_mut(d_means2d), &opt, stream);
      rc_check(rc, "gsr_backward", true);
    } else if (want_views) {
      d_views = at::zeros({v, kViewFloats}, f32);
    }
    std::vector<Tensor> out{d_means, d_cov, d_opac, d_colors, d_extra, d_means2d, d_views};
    // (after the launches: the device works on the backward while the host waits for the forward's status, if it has to)
    if (verify_own_forward(saved.token)) {  // the forward had overflowed (deferred status, default policy): NaN, not numbers
      const float qnan = std::numeric_limits<float>::quiet_NaN();
      for (Tensor& t : out)
        if (t.defined()) t.fill_(qnan);
    }
    return out;
  }

  Sizes sized(const Cfg& cfg, int64_t capacity) {
    const auto key = std::make_pair(cfg, capacity);
    {
      std::lock_guard<std::mutex> g(mu_);
      auto it = sizes_.find(key);
      if (it != sizes_.end()) return it->second;
    }
    const GsrDims d = cfg.dims(capacity);
    Sizes sz;
    const int rc = g_abi.workspace_sizes(&d, &sz.geom, &sz.bin, &sz.img);
    if (rc != 0) throw std::runtime_error("gsr_workspace_sizes rejected the call (code " + std::to_string(rc) + ")");
    sz.scratch = g_abi.backward_scratch_bytes(&d);
    std::lock_guard<std::mutex> g(mu_);
    if (sizes_.size() >= 64) sizes_.clear();
    sizes_[key] = sz;
    return sz;
  }

  // outputs + ONE allocation for the three workspaces, sliced on 2 MiB boundaries (as separate large allocations would sit; the
  // library lays geom's own sub-arrays out on such boundaries too).  reuse: the workspaces come from a per-(shape, stream) cache.
  // one_view (V = 1): the image as (3, H, W) and the radii as (N) - what the per-view operator returns - instead of views of them
  Plan make_plan(const Cfg& cfg, const at::Device& dev, int64_t capacity, bool reuse, bool one_view = false) {
    const Sizes sz = sized(cfg, capacity);
    Plan p;
    p.dims = cfg.launch_dims(capacity);
    const auto u8 = at::TensorOptions().dtype(at::kByte).device(dev);
    const auto f32 = u8.dtype(at::kFloat);
    Tensor whole;
    const auto ckey = std::make_tuple(cfg, capacity, (int)dev.index(), (uintptr_t)stream_of(dev));
    if (reuse) {
      std::lock_guard<std::mutex> g(mu_);
      auto it = ws_cache_.find(ckey);
      if (it != ws_cache_.end()) whole = it->second;
    }
    const int64_t al = (2 << 20) - 1;
    const int64_t o_g = ((int64_t)sz.bin + al) & ~al, o_i = o_g + (((int64_t)sz.geom + al) & ~al);
    if (!whole.defined()) {
      whole = at::empty({o_i + (int64_t)sz.img}, u8);
      if (reuse) {
        std::lock_guard<std::mutex> g(mu_);
        if (ws_cache_.size() >= 8) ws_cache_.clear();
        ws_cache_[ckey] = whole;
      }
    }
    p.bin = whole.narrow(0, 0, (int64_t)sz.bin);
    p.geom = whole.narrow(0, o_g, (int64_t)sz.geom);
    p.img = whole.narrow(0, o_i, (int64_t)sz.img);
    if (one_view && cfg.num_views == 1 && !cfg.has_extra && !cfg.alpha) {
      p.color = at::empty({3, cfg.height, cfg.width}, f32);
      p.radii = at::empty({cfg.num_gaussians}, u8.dtype(at::kInt));
      return p;
    }
    p.color = at::empty({cfg.num_views, 3, cfg.height, cfg.width}, f32);
    if (cfg.has_extra) p.extra_img = at::empty({cfg.num_views, cfg.height, cfg.width}, f32);
    if (cfg.alpha) p.alpha_img = at::empty({cfg.num_views, cfg.height, cfg.width}, f32);
    p.radii = at::empty({cfg.num_views, cfg.num_gaussians}, u8.dtype(at::kInt));
    return p;
  }

 private:
  int64_t default_capacity(const Cfg& cfg) {
    const ShapeKey key{cfg.num_views, cfg.num_gaussians, cfg.height, cfg.width};
    std::lock_guard<std::mutex> g(mu_);
    auto it = hint_.find(key);
    if (it != hint_.end()) return it->second;
    return (int64_t)cfg.num_views * std::max<int64_t>(8 * (int64_t)cfg.num_gaussians, 1 << 18);
  }

  void run_forward(Plan& p, const Cfg& cfg, const Tensor& viewbuf, const Tensor& means, const Tensor& cov, const Tensor& opac, const Tensor& colors,
                   const Tensor& extra, const Tensor& frames, hipStream_t stream) {
    const GsrView* vb = reinterpret_cast<const GsrView*>(viewbuf.data_ptr<float>());
    const Tensor fr = cfg.scale_rot ? frames_arg(cfg, frames) : Tensor();
    const GsrForwardOptions opt = launch_options<GsrForwardOptions>(cfg, fr, p.alpha_img);
    const int rc = g_abi.forward_ex(&p.dims, vb, fptr(means), fptr(cov), fptr(opac), fptr(colors), fptr(extra), p.color.data_ptr<float>(), fptr_mut(p.extra_img),
                                    p.radii.data_ptr<int32_t>(), p.geom.data_ptr(), p.bin.data_ptr(), p.img.data_ptr(), &opt, stream);
    rc_check(rc, "gsr_forward", false);
  }

  Pinned status_copy(const Tensor& bin, hipStream_t stream) {
    Pinned host;
    {
      std::lock_guard<std::mutex> g(mu_);
      if (!pool_.empty()) { host = pool_.back(); pool_.pop_back(); }
    }
    if (host.q == nullptr) {
      void* ptr = nullptr;
      TORCH_CHECK(hipHostMalloc(&ptr, 16, hipHostMallocDefault) == hipSuccess, "hipHostMalloc of a status buffer failed");
      host.q = reinterpret_cast<volatile int64_t*>(ptr);
    }
    host.arm();
    TORCH_CHECK(hipMemcpyAsync((void*)host.q, bin.data_ptr(), 16, hipMemcpyDeviceToHost, stream) == hipSuccess, "status copy could not be enqueued");
    return host;
  }

  // A short poll (a blocking call sleeps and wakes up 30-60 us late), bounded: after spin_us the wait becomes a device synchronize,
  // which sleeps instead of spinning and REPORTS a device fault or a stream error.
  void wait_status(const Pinned& host, int device) {
    if (host.arrived()) return;
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::nanoseconds((int64_t)(spin_us.load() * 1e3));
    while (!host.arrived()) {
      if (std::chrono::steady_clock::now() > deadline) {
        c10::hip::HIPGuard guard(device);
        hipError_t e;
        if (PyGILState_Check()) {  // (the forward is called from Python; the backward from one of the engine's threads, which hold no GIL)
          pybind11::gil_scoped_release nogil;
          e = hipDeviceSynchronize();
        } else {
          e = hipDeviceSynchronize();
        }
        if (e != hipSuccess) throw std::runtime_error(std::string("gsr_forward: the device reported an error while its status block was awaited: ") + hipGetErrorString(e));
        if (!host.arrived()) throw std::runtime_error("gsr_forward: the status block's copy did not execute (was the forward issued under stream capture?)");
        return;
      }
    }
  }

  Status take_status(Pinned host) {
    Status st;
    st.num_pairs = host.q[0];
    st.overflow = host.w()[2];
    st.max_list = host.w()[3];
    std::lock_guard<std::mutex> g(mu_);
    pool_.push_back(host);
    return st;
  }

  // What a shape's pair counts have looked like so far (Welford), and the largest count / longest list among them
  struct ShapeStats {
    int64_t n = 0, max_pairs = 0;
    int max_list = 0;
    double mean = 0.0, m2 = 0.0;
  };
  double factor_of(const ShapeStats& s) const {
    const double lo = headroom_min, hi = headroom_max;
    double f = lo;
    if (s.n >= 2 && s.mean > 0.0) f = std::max(f, 1.0 + headroom_sigmas * std::sqrt(s.m2 / (double)(s.n - 1)) / s.mean);
    return std::min(f, std::max(hi, lo));
  }

  // The capacity hint of a shape = what its largest pair count (and longest list) seen so far needs, times the head-room factor.  A
  // loop over one scene sees sigma = 0 and keeps 1.25x; a training run that meets a new scene every step widens the factor to
  // 1 + 4 sigma / mean (capped at 3x) - head-room costs workspace bytes, not time, and a deferred forward that outgrows it costs a step.
  void note_status(const ShapeKey& key, const Cfg& cfg, const Status& st) {
    Status top;
    double f;
    {
      std::lock_guard<std::mutex> g(mu_);
      ShapeStats& s = stats_[key];
      s.n += 1;
      const double d = (double)st.num_pairs - s.mean;
      s.mean += d / (double)s.n;
      s.m2 += d * ((double)st.num_pairs - s.mean);
      s.max_pairs = std::max(s.max_pairs, st.num_pairs);
      s.max_list = std::max(s.max_list, st.max_list);
      top.num_pairs = s.max_pairs; top.max_list = s.max_list;
      f = factor_of(s);
    }
    const int64_t need = capacity_for(cfg, top, f);
    std::lock_guard<std::mutex> g(mu_);
    last_ = st;
    has_status_ = true;
    seen_[key] += 1;
    int64_t& h = hint_[key];
    h = std::max(h, need);  // a running maximum: it never shrinks
  }

  std::mutex mu_;
  std::map<ShapeKey, int64_t> hint_, seen_;
  std::map<ShapeKey, ShapeStats> stats_;
  std::vector<PendingItem> pending_;
  std::set<int64_t> poisoned_;
  int64_t token_ = 0;
  Status last_;
  bool has_status_ = false;
  std::vector<Pinned> pool_;
  std::map<std::pair<Cfg, int64_t>, Sizes> sizes_;
  std::map<std::tuple<Cfg, int64_t, int, uintptr_t>, Tensor> ws_cache_;
};

// ---- autograd ---------------------------------------------------------------------------------------------------------------
struct RasterizeFn : public torch::autograd::Function<RasterizeFn> {
  // What the node keeps besides its saved tensors, under one capsule (any intrusive_ptr target, no class registration needed).  It lives with
  // the node (freed with the graph), past a first backward: a second one (retain_graph=True, several autograd.grad calls) runs on the same workspaces.
  struct State : torch::CustomClassHolder {
    Cfg cfg;
    Saved ws;  // the workspaces and the token of the forward
    Tensor frames;  // (undefined: none)
    std::shared_ptr<Backend> holder;  // (keeps the backend alive for as long as a graph can call back into it)
    size_t viewbuf_edge = 0;  // (needs_input_grad counts the Tensor arguments that are there: the camera records' position among them)
    int64_t camera_gradient = 1;
    bool want_means2d = false, rows_fresh = false;  // rows_fresh: the accumulator rows were zero-filled by the forward, usable once
  };
  // inputs: means, cov, opac, colors, extra (may be undefined), means2d (may be undefined: only its gradient is wanted), viewbuf
  // (optional inputs travel as std::optional: the engine records layout / device of every Tensor argument, an undefined one has none)
  static torch::autograd::variable_list forward(torch::autograd::AutogradContext* ctx, Tensor means, Tensor cov, Tensor opac, Tensor colors,
                                                c10::optional<Tensor> extra_o, c10::optional<Tensor> means2d_o, Tensor viewbuf, c10::optional<Tensor> frames_o,
                                                std::shared_ptr<Backend> holder, Cfg cfg, int64_t camera_gradient) {
    const Tensor extra = extra_o.has_value() ? *extra_o : Tensor(), means2d = means2d_o.has_value() ? *means2d_o : Tensor();
    auto st = c10::make_intrusive<State>();
    st->cfg = cfg; st->holder = holder; st->camera_gradient = camera_gradient; st->frames = frames_o.has_value() ? *frames_o : Tensor();
    st->viewbuf_edge = 4 + (extra.defined() ? 1 : 0) + (means2d.defined() ? 1 : 0);
    st->want_means2d = means2d.defined(); st->rows_fresh = (cfg.flags & GSR_FLAG_BACKWARD_FOLLOWS) != 0;
    ForwardOut o = holder->forward(cfg, viewbuf, means, cov, opac, colors, extra, st->frames, -1, false);
    st->ws = o.saved; ctx->saved_data["state"] = c10::IValue::make_capsule(st);
    ctx->save_for_backward({means, cov, opac, colors, extra.defined() ? extra : at::empty({0}, means.options()), viewbuf});
    Tensor extra_img = o.extra_img;
    ctx->mark_non_differentiable({o.radii});
    if (!extra_img.defined()) {
      extra_img = at::empty({0}, o.color.options());
      ctx->mark_non_differentiable({extra_img});
    }
    if (cfg.alpha) {  // a third differentiable output, only when asked for
      // an output the loss does not use arrives in backward() as an undefined tensor instead of a materialised image of zeros: an alpha
      // image that was only looked at then costs the backward nothing (a NULL dL_dalpha_img: the instances without alpha)
      ctx->set_materialize_grads(false);
      return {o.color, extra_img, o.radii, o.alpha_img};
    }
    return {o.color, extra_img, o.radii};
  }

  static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const Tensor &means = saved[0], &cov = saved[1], &opac = saved[2], &colors = saved[3], &viewbuf = saved[5];
    const auto st = c10::static_intrusive_pointer_cast<State>(ctx->saved_data["state"].toCapsule());
    const Cfg& cfg = st->cfg;
    Tensor extra = saved[4], g_color = grads[0], g_extra = grads[1];
    if (!cfg.has_extra) { extra = Tensor(); g_extra = Tensor(); }
    else if (cfg.extra_mode()) extra = Tensor();  // built-in mode: no extra array; its gradient is folded into d_means by the backward kernel
    if (!g_color.defined()) g_color = at::zeros({cfg.num_views, 3, cfg.height, cfg.width}, means.options().dtype(at::kFloat));
    const bool cam = ctx->needs_input_grad(st->viewbuf_edge);  // cameras being learned (PF3plat's pose refinement): opt-in, SURVEY 8f-3
    // (GSR_FLAG_FOV_GRADIENT in the call's flags - saved.dims carry it into the backward's launch and the partials' size - implies
    // the full camera gradient: the depth term alone has no tan-fov columns)
    const int want_views = cam ? ((st->camera_gradient == 2 && !(cfg.flags & GSR_FLAG_FOV_GRADIENT)) ? 2 : 1) : 0;
    std::vector<Tensor> g = st->holder->backward(cfg, st->ws, viewbuf, means, cov, opac, colors, extra, g_color, g_extra, st->want_means2d, st->rows_fresh,
                                                 st->frames, want_views, (cfg.alpha && grads.size() > 3) ? grads[3] : Tensor());
    st->rows_fresh = false;  // (the workspaces stay: a second backward runs on them again, as upstream's Function can)
    return {g[0], g[1], g[2], g[3], g[4], g[5], g[6], Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// Camera records from camera-to-world extrinsics with a gradient path back to the extrinsics: one launch each way.
Tensor setup_views_raw(const Tensor& extrinsics, const Tensor& intrinsics, const Tensor& near, const Tensor& far, const Tensor& background, bool scale_invariant) {
  check_device({&extrinsics, &intrinsics, &near, &far, &background});
  const int64_t v = extrinsics.size(0);
  const Tensor ext = f32c(extrinsics), intr = f32c(intrinsics), nr = f32c(near), fr = f32c(far), bg = f32c(background);
  Tensor out = at::empty({v, kViewFloats}, ext.options());
  c10::hip::HIPGuard guard(ext.device().index());
  const int rc = g_abi.setup_views((int)v, fptr(ext), fptr(intr), fptr(nr), fptr(fr), fptr(bg), bg.dim() == 2 ? 3 : 0, scale_invariant ? 1 : 0,
                                   reinterpret_cast<GsrView*>(out.data_ptr<float>()), stream_of(ext.device()));
  if (rc != 0) throw std::runtime_error("gsr_setup_views failed with code " + std::to_string(rc));
  return out;
}

// (V, 48) camera records + their gradient -> dL/d extrinsics (V, 4, 4), fp32 (gsr_setup_views_backward: fp64 inside)
Tensor setup_views_backward(const Tensor& viewbuf, const Tensor& d_views) {
  check_device({&viewbuf, &d_views});
  const Tensor vb = f32c(viewbuf), dv = f32c(d_views);
  Tensor out = at::empty({vb.size(0), 4, 4}, vb.options());
  c10::hip::HIPGuard guard(vb.device().index());
  const int rc = g_abi.setup_views_backward((int)vb.size(0), reinterpret_cast<const GsrView*>(vb.data_ptr<float>()), fptr(dv), out.data_ptr<float>(), stream_of(vb.device()));
  if (rc != 0) throw std::runtime_error("gsr_setup_views_backward failed with code " + std::to_string(rc));
  return out;
}

// ... and with the intrinsics' share: (V, 3, 3) through get_fov's arithmetic (gsr_setup_views_backward_ex, one launch for both).
// Either result is undefined where it is not wanted.
std::tuple<Tensor, Tensor> setup_views_backward_ex(const Tensor& viewbuf, const Tensor& intrinsics, const Tensor& d_views, bool want_ext, bool want_intr) {
  check_device({&viewbuf, &intrinsics, &d_views});
  const Tensor vb = f32c(viewbuf), intr = f32c(intrinsics), dv = f32c(d_views);
  TORCH_CHECK(intr.numel() == vb.size(0) * 9, "intrinsics must be (views, 3, 3)");
  Tensor d_ext, d_intr;
  if (want_ext) d_ext = at::empty({vb.size(0), 4, 4}, vb.options());
  if (want_intr) d_intr = at::empty({vb.size(0), 3, 3}, vb.options());
  c10::hip::HIPGuard guard(vb.device().index());
  const int rc = g_abi.setup_views_backward_ex((int)vb.size(0), reinterpret_cast<const GsrView*>(vb.data_ptr<float>()), fptr(intr), fptr(dv), fptr_mut(d_ext),
                                               fptr_mut(d_intr), stream_of(vb.device()));
  if (rc != 0) throw std::runtime_error("gsr_setup_views_backward_ex failed with code " + std::to_string(rc));
  return {d_ext, d_intr};
}

struct SetupViewsFn : public torch::autograd::Function<SetupViewsFn> {
  struct State : torch::CustomClassHolder { at::ScalarType ext_dtype, intr_dtype; };  // what the two gradients are handed back as
  static Tensor forward(torch::autograd::AutogradContext* ctx, Tensor extrinsics, Tensor intrinsics, Tensor near, Tensor far, Tensor background, bool scale_invariant) {
    Tensor vb = setup_views_raw(extrinsics, intrinsics, near, far, background, scale_invariant);
    ctx->save_for_backward({vb, intrinsics});
    auto st = c10::make_intrusive<State>();
    st->ext_dtype = extrinsics.scalar_type(); st->intr_dtype = intrinsics.scalar_type();
    ctx->saved_data["state"] = c10::IValue::make_capsule(st);
    return vb;
  }
  static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const auto st = c10::static_intrusive_pointer_cast<State>(ctx->saved_data["state"].toCapsule());
    const bool want_ext = ctx->needs_input_grad(0), want_intr = ctx->needs_input_grad(1);
    Tensor d_ext, d_intr;
    if (want_intr) {
      std::tie(d_ext, d_intr) = setup_views_backward_ex(saved[0], saved[1], grads[0], want_ext, true);
      d_intr = d_intr.to(st->intr_dtype).reshape(saved[1].sizes());
    } else if (want_ext) {
      d_ext = setup_views_backward(saved[0], grads[0]);
    }
    if (d_ext.defined()) d_ext = d_ext.to(st->ext_dtype);
    return {d_ext, d_intr, Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// pose_gradients / intrinsics_gradients: which of the two camera inputs keeps a gradient path (each only if it requires one; the
// other goes in detached)
Tensor views_from_cameras(const Tensor& extrinsics, const Tensor& intrinsics, const Tensor& near, const Tensor& far, const Tensor& background, bool scale_invariant,
                          bool pose_gradients, bool intrinsics_gradients) {
  const bool grad = at::GradMode::is_enabled();
  const bool ext = pose_gradients && grad && extrinsics.requires_grad(), intr = intrinsics_gradients && grad && intrinsics.requires_grad();
  if (ext || intr)
    return SetupViewsFn::apply(ext ? extrinsics : extrinsics.detach(), intr ? intrinsics : intrinsics.detach(), near, far, background, scale_invariant);
  at::NoGradGuard ng;
  return setup_views_raw(extrinsics, intrinsics, near, far, background, scale_invariant);
}

// Cameras of the reference's fake orthographic render (cuda_splatting.py:153-181) in one launch: -> (V, 48) records and the (V, 20)
// values after the move (extrinsics 16, fov_x, fov_y, near, far)
std::tuple<Tensor, Tensor> setup_views_orthographic(const Tensor& extrinsics, const Tensor& width, const Tensor& height, const Tensor& near, const Tensor& far,
                                                    const Tensor& background, double fov_degrees) {
  check_device({&extrinsics, &width, &height, &near, &far, &background});
  const int64_t v = extrinsics.size(0);
  const Tensor ext = f32c(extrinsics), wd = f32c(width).reshape({v}), ht = f32c(height).reshape({v}), nr = f32c(near).reshape({v}),
               fr = f32c(far).reshape({v}), bg = f32c(background);
  Tensor out = at::empty({v, kViewFloats}, ext.options()), dump = at::empty({v, 20}, ext.options());
  c10::hip::HIPGuard guard(ext.device().index());
  const int rc = g_abi.setup_views_orthographic((int)v, fptr(ext), fptr(wd), fptr(ht), fptr(nr), fptr(fr), fptr(bg), bg.dim() == 2 ? 3 : 0, (float)fov_degrees,
                                                reinterpret_cast<GsrView*>(out.data_ptr<float>()), dump.data_ptr<float>(), stream_of(ext.device()));
  if (rc != 0) throw std::runtime_error("gsr_setup_views_orthographic failed with code " + std::to_string(rc));
  return {out, dump};
}

// upstream's GaussianRasterizer.markVisible: (S, N) uint8, 1 where the Gaussian passes the near-plane test of view 0 of its set
Tensor mark_visible(const Cfg& cfg, const Tensor& viewbuf, const Tensor& means) {
  check_device({&viewbuf, &means});
  const Tensor vb = f32c(viewbuf), m = f32c(means);
  Tensor present = at::empty({cfg.num_sets, cfg.num_gaussians}, m.options().dtype(at::kByte));
  const GsrDims d = cfg.dims(0);
  c10::hip::HIPGuard guard(m.device().index());
  const int rc = g_abi.mark_visible(&d, reinterpret_cast<const GsrView*>(vb.data_ptr<float>()), m.data_ptr<float>(), present.data_ptr<uint8_t>(), stream_of(m.device()));
  if (rc != 0) throw std::runtime_error("gsr_mark_visible failed with code " + std::to_string(rc));
  return present;
}

// upstream's scales= / rotations= form: covariances (n, 6) from scales (n, 3) and quaternions (n, 4; r, x, y, z), and their backward
Tensor cov_from_scale_rot(const Tensor& scales_in, const Tensor& rotations_in, double scale_modifier) {
  check_device({&scales_in, &rotations_in});
  const Tensor scales = f32c(scales_in), rotations = f32c(rotations_in);
  const int64_t n = scales.size(0);
  TORCH_CHECK(scales.numel() == 3 * n && rotations.numel() == 4 * n, "cov_from_scale_rot: scales (n, 3) and rotations (n, 4) expected");
  Tensor out = at::empty({n, 6}, scales.options());
  c10::hip::HIPGuard guard(scales.device().index());
  const int rc = g_abi.cov_from_scale_rot(n, fptr(scales), fptr(rotations), (float)scale_modifier, out.data_ptr<float>(), stream_of(scales.device()));
  if (rc != 0) throw std::runtime_error("gsr_cov_from_scale_rot failed with code " + std::to_string(rc));
  return out;
}
std::tuple<Tensor, Tensor> cov_from_scale_rot_backward(const Tensor& scales_in, const Tensor& rotations_in, double scale_modifier, const Tensor& d_cov6_in) {
  check_device({&scales_in, &rotations_in, &d_cov6_in});
  const Tensor scales = f32c(scales_in), rotations = f32c(rotations_in), d_cov6 = f32c(d_cov6_in);
  const int64_t n = scales.size(0);
  TORCH_CHECK(scales.numel() == 3 * n && rotations.numel() == 4 * n && d_cov6.numel() == 6 * n,
              "cov_from_scale_rot_backward: scales (n, 3), rotations (n, 4) and d_cov6 (n, 6) expected");
  Tensor d_s = at::empty_like(scales), d_r = at::empty_like(rotations);
  c10::hip::HIPGuard guard(scales.device().index());
  const int rc = g_abi.cov_from_scale_rot_backward(n, fptr(scales), fptr(rotations), (float)scale_modifier, fptr(d_cov6), d_s.data_ptr<float>(),
                                                   d_r.data_ptr<float>(), stream_of(scales.device()));
  if (rc != 0) throw std::runtime_error("gsr_cov_from_scale_rot_backward failed with code " + std::to_string(rc));
  return {d_s, d_r};
}

// The (1, 48) camera record of one upstream settings object in ONE launch (gsr_pack_view): the matrices, the camera centre (read
// through its stride: the reference passes `extrinsics[i, :3, 3]`, stride 4) and the background stay where they are on the device;
// the tan-fovs travel as launch arguments (floats) or as device pointers (tensors, as the orthographic wrapper passes them).
Tensor pack_view(const Tensor& viewmatrix, const Tensor& projmatrix, const Tensor& campos_in, const Tensor& bg_in, double tanfovx, double tanfovy, const Tensor& tanfovx_t,
                 const Tensor& tanfovy_t, double scale_modifier, const at::Device& device) {
  const auto to_dev = [&](const Tensor& t) { return (t.device() == device && t.scalar_type() == at::kFloat) ? t : t.to(device, at::kFloat); };
  const Tensor vm = to_dev(viewmatrix).contiguous(), pm = to_dev(projmatrix).contiguous(), bg = to_dev(bg_in).contiguous();
  Tensor cp = to_dev(campos_in);
  if (cp.dim() != 1 || cp.size(0) != 3) cp = cp.reshape({3});
  check_device({&vm, &pm, &bg, &cp});
  Tensor txd, tyd;
  if (tanfovx_t.defined()) txd = to_dev(tanfovx_t.reshape({-1}).narrow(0, 0, 1));
  if (tanfovy_t.defined()) tyd = to_dev(tanfovy_t.reshape({-1}).narrow(0, 0, 1));
  Tensor out = at::empty({1, kViewFloats}, vm.options());
  c10::hip::HIPGuard guard(device.index());
  const int rc = g_abi.pack_view(fptr(vm), fptr(pm), fptr(cp), (int)cp.stride(0), fptr(bg), (float)tanfovx, (float)tanfovy, fptr(txd), fptr(tyd), (float)scale_modifier,
                                 reinterpret_cast<GsrView*>(out.data_ptr<float>()), stream_of(device));
  if (rc != 0) throw std::runtime_error("gsr_pack_view failed with code " + std::to_string(rc));
  return out;
}

// ---- the Gaussian adapter (gsr_adapt / gsr_adapt_backward_ex): one autograd node around the two calls ------------------------------
// raw (..., 7 + 3 M) is read where it is: its rows must lie a constant number of floats apart (the encoder's `gaussians[..., 2:]`
// slice of an 84-wide tensor does: stride 84); only a tensor whose leading dims do not collapse to one row stride is copied.
bool rows_evenly_spaced(const Tensor& t, int64_t* row_stride) {
  *row_stride = t.size(-1);
  if (t.dim() < 2 || (t.size(-1) > 1 && t.stride(-1) != 1)) return false;
  int64_t expect = -1;
  for (int64_t d = t.dim() - 2; d >= 0; --d) {
    if (t.size(d) == 1) continue;  // (the stride of a dim of one entry says nothing)
    if (expect < 0) {
      expect = *row_stride = t.stride(d);
      if (expect < t.size(-1)) return false;
    } else if (t.stride(d) != expect) {
      return false;
    }
    expect *= t.size(d);
  }
  return true;
}
struct AdaptFn : public torch::autograd::Function<AdaptFn> {
  struct State : torch::CustomClassHolder {  // the forward's launch arguments, for the backward's launch, and the shapes two gradients go back in
    int64_t g, p, row_stride, degree, height, width;
    double lo, hi, eps;
    std::vector<int64_t> raw_sizes, coord_sizes;  // (of raw and coordinates as they were given)
  };
  static torch::autograd::variable_list forward(torch::autograd::AutogradContext* ctx, Tensor extrinsics, Tensor intrinsics, Tensor coordinates, Tensor depths,
                                                Tensor raw_in, double lo, double hi, int64_t height, int64_t width, double eps, int64_t degree) {
    check_device({&extrinsics, &intrinsics, &coordinates, &depths, &raw_in});
    TORCH_CHECK(degree >= 0 && degree <= 4, "adapt: sh_degree must be 0..4, got ", degree);
    const int64_t m = (degree + 1) * (degree + 1), rowf = 7 + 3 * m;
    for (const Tensor* t : {&extrinsics, &intrinsics, &coordinates, &depths, &raw_in})
      TORCH_CHECK(t->scalar_type() == at::kFloat, "adapt: float32 tensors expected");
    TORCH_CHECK(extrinsics.dim() == 3 && extrinsics.size(1) == 4 && extrinsics.size(2) == 4, "adapt: extrinsics (G, 4, 4) expected");
    const int64_t g = extrinsics.size(0);
    TORCH_CHECK(intrinsics.dim() == 3 && intrinsics.size(0) == g && intrinsics.size(1) == 3 && intrinsics.size(2) == 3, "adapt: intrinsics (G, 3, 3) expected");
    TORCH_CHECK(depths.dim() == 2 && depths.size(0) == g, "adapt: depths (G, P) expected");
    const int64_t p = depths.size(1);
    TORCH_CHECK(g < (1 << 30) && p < (1 << 30), "adapt: too many Gaussians for one call");
    TORCH_CHECK(coordinates.numel() == g * p * 2 && coordinates.size(-1) == 2, "adapt: coordinates (G, P, 2) expected");
    TORCH_CHECK(raw_in.dim() >= 2 && raw_in.size(-1) == rowf && raw_in.numel() == g * p * rowf, "adapt: raw (G, P, ", rowf, ") expected");
    const Tensor ext = extrinsics.contiguous(), intr = intrinsics.contiguous(), coords = coordinates.contiguous(), dep = depths.contiguous();
    int64_t row_stride = rowf;
    const bool in_place = rows_evenly_spaced(raw_in, &row_stride);
    const Tensor raw = in_place ? raw_in : raw_in.contiguous();
    if (!in_place) row_stride = rowf;
    Tensor means = at::empty({g, p, 3}, ext.options()), records = at::empty({g, p, 7}, ext.options()), harmonics = at::empty({g, p, 3, m}, ext.options());
    c10::hip::HIPGuard guard(ext.device().index());
    const int rc = g_abi.adapt((int)g, (int)p, (int)degree, fptr(ext), fptr(intr), fptr(coords), fptr(dep), fptr(raw), row_stride, (float)lo, (float)hi,
                               (int)height, (int)width, (float)eps, means.data_ptr<float>(), records.data_ptr<float>(), harmonics.data_ptr<float>(), stream_of(ext.device()));
    if (rc != 0) throw std::runtime_error("gsr_adapt failed with code " + std::to_string(rc));
    ctx->save_for_backward({ext, intr, coords, dep, raw});
    auto st = c10::make_intrusive<State>();
    st->g = g; st->p = p; st->row_stride = row_stride; st->degree = degree; st->height = height; st->width = width; st->lo = lo; st->hi = hi; st->eps = eps;
    st->raw_sizes = raw_in.sizes().vec(); st->coord_sizes = coordinates.sizes().vec();
    ctx->saved_data["state"] = c10::IValue::make_capsule(st);
    return {means, records, harmonics};
  }
  static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const Tensor &ext = saved[0], &intr = saved[1], &coords = saved[2], &dep = saved[3], &raw = saved[4];
    const auto st = c10::static_intrusive_pointer_cast<State>(ctx->saved_data["state"].toCapsule());
    const int64_t g = st->g, p = st->p, degree = st->degree, m = (degree + 1) * (degree + 1);
    check_device({&grads[0], &grads[1], &grads[2]});
    const Tensor d_means = f32c(grads[0]), d_rec = f32c(grads[1]), d_harm = f32c(grads[2]);
    Tensor d_raw = at::empty({g, p, 7 + 3 * m}, ext.options()), d_dep = at::empty({g, p}, ext.options()), d_coords = at::empty({g, p, 2}, ext.options());
    Tensor d_ext = g * p > 0 ? at::empty({g, 4, 4}, ext.options()) : at::zeros({g, 4, 4}, ext.options());
    c10::hip::HIPGuard guard(ext.device().index());
    // intrinsics being learned: their gradient comes out of the same two launches (wider partial rows); otherwise NULL, which is gsr_adapt_backward
    const bool want_intr = ctx->needs_input_grad(1);
    Tensor d_intr = !want_intr ? Tensor() : g * p > 0 ? at::empty({g, 3, 3}, ext.options()) : at::zeros({g, 3, 3}, ext.options());
    Tensor partials = at::empty({(int64_t)g_abi.adapt_partials_bytes_ex((int)g, (int)p, want_intr ? 1 : 0)}, ext.options().dtype(at::kByte));
    const int rc = g_abi.adapt_backward_ex((int)g, (int)p, (int)degree, fptr(ext), fptr(intr), fptr(coords), fptr(dep), fptr(raw), st->row_stride, (float)st->lo, (float)st->hi,
                                        (int)st->height, (int)st->width, (float)st->eps, fptr(d_means), fptr(d_rec), fptr(d_harm), d_raw.data_ptr<float>(),
                                        d_dep.data_ptr<float>(), d_coords.data_ptr<float>(), d_ext.data_ptr<float>(), fptr_mut(d_intr),
                                        reinterpret_cast<float*>(partials.data_ptr<uint8_t>()), stream_of(ext.device()));
    if (rc != 0) throw std::runtime_error("gsr_adapt_backward_ex failed with code " + std::to_string(rc));
    return {d_ext, d_intr, d_coords.reshape(st->coord_sizes), d_dep, d_raw.reshape(st->raw_sizes), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};
std::tuple<Tensor, Tensor, Tensor> adapt(const Tensor& extrinsics, const Tensor& intrinsics, const Tensor& coordinates, const Tensor& depths, const Tensor& raw, double lo,
                                         double hi, int64_t height, int64_t width, double eps, int64_t degree) {
  auto out = AdaptFn::apply(extrinsics, intrinsics, coordinates, depths, raw, lo, hi, height, width, eps, degree);
  return {out[0], out[1], out[2]};
}

// ---- what Python calls ------------------------------------------------------------------------------------------------------
struct PyBackend {
  std::shared_ptr<Backend> holder = std::make_shared<Backend>();
  Backend& be() { return *holder; }
};

pybind11::dict status_dict(const Status& st) {
  pybind11::dict d;
  d["num_pairs"] = st.num_pairs;
  d["overflow"] = st.overflow;
  d["max_list"] = st.max_list;
  return d;
}

// (color, extra_img (undefined without the extra channel), radii): the differentiable operator - an autograd node only when the call
// announces a backward.  Runs WITHOUT the GIL (the callers below release it around their work and take it back to build the result):
// a blocking forward polls its status block for as long as its kernels run, and other Python threads - a data loader's pin-memory
// thread - must not stand still meanwhile.  (`saved` of the result stays empty: the node keeps the workspaces.)
ForwardOut rasterize_impl(PyBackend& pb, const Tensor& means, const Tensor& cov, const Tensor& opac, const Tensor& colors, const c10::optional<Tensor>& extra,
                          const c10::optional<Tensor>& means2d, const Tensor& viewbuf, const Cfg& cfg, const c10::optional<Tensor>& frames, int64_t camera_gradient) {
  const Tensor ex = extra.has_value() ? *extra : Tensor(), fr = frames.has_value() ? *frames : Tensor();
  // nothing here can be differentiated: no autograd node, no saved workspaces
  if (!(cfg.flags & GSR_FLAG_BACKWARD_FOLLOWS)) return pb.be().forward(cfg, viewbuf, means, cov, opac, colors, ex, fr, -1, true);
  auto out = RasterizeFn::apply(means, cov, opac, colors, extra, means2d, viewbuf, frames, pb.holder, cfg, camera_gradient);
  return {out[0], cfg.has_extra ? out[1] : Tensor(), out[2], {}, cfg.alpha ? out[3] : Tensor()};
}
pybind11::object or_none(const Tensor& t) { return t.defined() ? pybind11::cast(t) : pybind11::none(); }
pybind11::tuple raster_tuple(const ForwardOut& r) {
  if (r.alpha_img.defined()) return pybind11::make_tuple(r.color, or_none(r.extra_img), r.radii, r.alpha_img);  // (only a call that asked for alpha gets four)
  return pybind11::make_tuple(r.color, or_none(r.extra_img), r.radii);
}
pybind11::tuple rasterize(PyBackend& pb, const Tensor& means, const Tensor& cov, const Tensor& opac, const Tensor& colors, const c10::optional<Tensor>& extra,
                          const c10::optional<Tensor>& means2d, const Tensor& viewbuf, const Cfg& cfg, const c10::optional<Tensor>& frames, int64_t camera_gradient) {
  const ForwardOut r = [&] { pybind11::gil_scoped_release nogil; return rasterize_impl(pb, means, cov, opac, colors, extra, means2d, viewbuf, cfg, frames, camera_gradient); }();
  return raster_tuple(r);
}

// The call shape of `rasterize_views`, stated ONCE: argument checks (message for message what the Python surface documents), dtype /
// contiguity normalisation, the call shape and its flags (GSR_FLAG_BACKWARD_FOLLOWS when something can be differentiated).  Touches no
// device: `rasterize_views` below runs it in front of the operator, and `pf3plat_amd.rasterizer` runs the SAME function (bound as
// `prepare_call`) in front of any other backend object - the tests slide the CPU oracle under the host wrappers that way - so the two
// paths cannot drift apart.
struct Prepared {
  Tensor means, cov, opac, colors, viewbuf;
  c10::optional<Tensor> extra, frames;
  Cfg cfg;  // (alpha stays off: the caller's to set)
};
Prepared prepare_call(const Tensor& means_in, const Tensor& cov_in, const Tensor& opac_in, const Tensor& colors_in, const Tensor& viewbuf_in, int64_t h, int64_t w,
                      int64_t sh_degree, bool use_sh, int64_t views_per_set, const c10::optional<Tensor>& extra_in, const c10::optional<Tensor>& means2d,
                      int64_t max_sh_eval, bool sh_planar, bool cov_3x3, int64_t extra_mode, bool debug, bool prefiltered, int64_t deterministic, bool scale_rot,
                      const c10::optional<Tensor>& frames_in, int64_t camera_gradient, int64_t sh_frame /* 0 none, 1 "rasterizer", 2 "e3nn" */) {
  Prepared p;
  const int64_t s = means_in.size(0), n = means_in.size(1), v = viewbuf_in.size(0);
  if (v != s * views_per_set) throw pybind11::value_error(std::to_string(v) + " views != " + std::to_string(s) + " sets x " + std::to_string(views_per_set) + " views per set");
  p.means = f32c(means_in); p.cov = f32c(cov_in); p.opac = f32c(opac_in); p.colors = f32c(colors_in);
  const Tensor &cov = p.cov, &colors = p.colors;
  if (extra_in.has_value() && extra_in->defined()) p.extra = f32c(*extra_in);
  if (use_sh && colors.dim() != 4) throw pybind11::value_error("shs must be (sets, N, M, 3) or (sets, N, 3, M)");
  const auto shape_str = [](const Tensor& t) { std::ostringstream o; o << t.sizes(); return o.str(); };
  if (scale_rot) {
    if (cov_3x3 || cov.dim() != 3 || cov.size(2) != 7) throw pybind11::value_error("scale/rotation records have shape " + shape_str(cov) + "; expected (sets, N, 7)");
    if (frames_in.has_value() && frames_in->defined()) p.frames = f32c(frames_in->detach());
  } else if (frames_in.has_value() && frames_in->defined()) {
    throw pybind11::value_error("`frames` goes with scale_rot=True");
  } else if (cov_3x3 ? (cov.dim() != 4 || cov.size(2) != 3 || cov.size(3) != 3) : (cov.dim() != 3 || cov.size(2) != 6)) {
    throw pybind11::value_error("covariances have shape " + shape_str(cov) + "; expected (sets, N, " + (cov_3x3 ? "3, 3" : "6") + ")");
  }
  const int64_t m = use_sh ? (sh_planar ? colors.size(3) : colors.size(2)) : 0;
  int64_t flags = ((sh_planar && use_sh) ? GSR_FLAG_SH_PLANAR : 0) | (cov_3x3 ? GSR_FLAG_COV_3X3 : 0);
  const bool det = deterministic < 0 ? at::globalContext().deterministicAlgorithms() : deterministic != 0;
  flags |= (debug ? GSR_FLAG_DEBUG : 0) | (prefiltered ? GSR_FLAG_PREFILTERED : 0) | (det ? GSR_FLAG_DETERMINISTIC : 0);
  const auto rg = [](const c10::optional<Tensor>& t) { return t.has_value() && t->defined() && t->requires_grad(); };
  if (at::GradMode::is_enabled() && (p.means.requires_grad() || cov.requires_grad() || p.opac.requires_grad() || colors.requires_grad() || rg(p.extra) || rg(means2d) ||
                                     viewbuf_in.requires_grad()))
    flags |= GSR_FLAG_BACKWARD_FOLLOWS;  // the forward zero-fills the backward's accumulator rows on its way
  if (extra_mode) {
    if (p.extra.has_value()) throw pybind11::value_error("give either `extra` or `extra_mode`");
    flags |= GSR_FLAG_EXTRA_MODE(extra_mode);
  }
  const bool has_extra = p.extra.has_value() || extra_mode != 0;
  if (camera_gradient != 1 && camera_gradient != 2) throw pybind11::value_error("camera_gradient must be 'full' or 'depth'");
  if (sh_frame < 0 || sh_frame > 2) throw pybind11::value_error("sh_frame must be None, 'rasterizer' or 'e3nn'");
  if (sh_frame) {  // harmonics in the frames' coordinates (GSR_FLAG_SH_IN_FRAME): the frames of the scale / rotation form
    if (!scale_rot || !p.frames.has_value()) throw pybind11::value_error("sh_frame needs scale_rot=True and `frames`");
    if (!use_sh) throw pybind11::value_error("sh_frame needs use_sh=True (harmonics)");
    flags |= GSR_FLAG_SH_IN_FRAME | (sh_frame == 2 ? GSR_FLAG_SH_FRAME_E3NN : 0);
  }
  Cfg& c = p.cfg;
  c.num_views = (int)v; c.num_sets = (int)s; c.views_per_set = (int)views_per_set; c.num_gaussians = (int)n; c.height = (int)h; c.width = (int)w;
  c.sh_degree = (int)sh_degree; c.sh_coeffs = (int)m; c.max_sh_eval = (int)max_sh_eval; c.has_extra = has_extra; c.flags = (int)flags; c.scale_rot = scale_rot;
  p.viewbuf = f32c(viewbuf_in);
  return p;
}

// `pf3plat_amd.rasterizer.rasterize_views` in one crossing: the call shape (prepare_call), then the operator.
pybind11::tuple rasterize_views(PyBackend& pb, const Tensor& means_in, const Tensor& cov_in, const Tensor& opac_in, const Tensor& colors_in, const Tensor& viewbuf_in,
                                int64_t h, int64_t w, int64_t sh_degree, bool use_sh, int64_t views_per_set, const c10::optional<Tensor>& extra_in,
                                const c10::optional<Tensor>& means2d, int64_t max_sh_eval, bool sh_planar, bool cov_3x3, int64_t extra_mode, bool debug,
                                bool prefiltered, int64_t deterministic, bool scale_rot, const c10::optional<Tensor>& frames_in, int64_t camera_gradient,
                                int64_t sh_frame, bool return_alpha, bool intrinsics_gradients) {
  ForwardOut result;
  {
  pybind11::gil_scoped_release nogil;
  Prepared p = prepare_call(means_in, cov_in, opac_in, colors_in, viewbuf_in, h, w, sh_degree, use_sh, views_per_set, extra_in, means2d, max_sh_eval, sh_planar,
                                  cov_3x3, extra_mode, debug, prefiltered, deterministic, scale_rot, frames_in, camera_gradient, sh_frame);
  p.cfg.alpha = return_alpha;
  // the tan-fov columns of the camera gradient (GSR_FLAG_FOV_GRADIENT): only where a backward will ask for the camera gradient at all
  if (intrinsics_gradients && (p.cfg.flags & GSR_FLAG_BACKWARD_FOLLOWS) && viewbuf_in.requires_grad()) p.cfg.flags |= GSR_FLAG_FOV_GRADIENT;
  result = rasterize_impl(pb, p.means, p.cov, p.opac, p.colors, p.extra, means2d, p.viewbuf, p.cfg, p.frames, camera_gradient);
  }
  return raster_tuple(result);
}

// The per-view operator with upstream's call shape (reference cuda_splatting.py:99-124: one settings object, one call per view) in ONE
// crossing from Python: the camera record (gsr_pack_view), the V = 1 views of the inputs, the call shape, the operator, the [0]s.
// tanfov*: floats, or tensors (the orthographic wrapper passes tensors); cov3d: (n, 6) or anything that reshapes to it.
pybind11::tuple rasterize_one_view(PyBackend& pb, int64_t height, int64_t width, double tanfovx, double tanfovy, const c10::optional<Tensor>& tanfovx_t,
                                   const c10::optional<Tensor>& tanfovy_t, const Tensor& bg, double scale_modifier, const Tensor& viewmatrix,
                                   const Tensor& projmatrix, int64_t sh_degree, const Tensor& campos, bool prefiltered, bool debug, const Tensor& means3d,
                                   const c10::optional<Tensor>& means2d, const Tensor& opacities, const c10::optional<Tensor>& shs,
                                   const c10::optional<Tensor>& colors_precomp, const Tensor& cov3d) {
  Tensor out_color, out_radii;
  {
  pybind11::gil_scoped_release nogil;
  const int64_t n = means3d.size(0);
  const bool use_sh = shs.has_value();
  const Tensor viewbuf = pack_view(viewmatrix, projmatrix, campos, bg, tanfovx, tanfovy, tanfovx_t.has_value() ? *tanfovx_t : Tensor(),
                                   tanfovy_t.has_value() ? *tanfovy_t : Tensor(), scale_modifier, means3d.device());
  const Tensor& col_in = use_sh ? *shs : *colors_precomp;
  if (use_sh && col_in.dim() != 3) throw pybind11::value_error("shs must be (N, M, 3)");
  TORCH_CHECK(cov3d.numel() == 6 * n && opacities.numel() == n, "cov3D_precomp must hold (N, 6) values and opacities N");
  Cfg cfg;  // V = 1, S = 1; (N, M, 3) harmonics or (N, 3) colours
  cfg.num_views = cfg.num_sets = cfg.views_per_set = 1; cfg.num_gaussians = (int)n; cfg.height = (int)height; cfg.width = (int)width;
  cfg.sh_degree = (int)sh_degree; cfg.sh_coeffs = use_sh ? (int)col_in.size(1) : 0;
  cfg.flags = (debug ? GSR_FLAG_DEBUG : 0) | (prefiltered ? GSR_FLAG_PREFILTERED : 0) | (at::globalContext().deterministicAlgorithms() ? GSR_FLAG_DETERMINISTIC : 0);
  const bool grad = at::GradMode::is_enabled() && (means3d.requires_grad() || cov3d.requires_grad() || opacities.requires_grad() || col_in.requires_grad() ||
                                                   (means2d.has_value() && means2d->defined() && means2d->requires_grad()));
  if (!grad) {
    // nothing can be differentiated (the reference's inference loop): the arrays go to the library as they are - the call shape says
    // V = 1, S = 1 - and the image / radii are allocated in the shapes the operator returns: no view op on either side of the call
    ForwardOut o = pb.be().forward(cfg, viewbuf, f32c(means3d), f32c(cov3d), f32c(opacities), f32c(col_in), Tensor(), Tensor(), -1, true, true);
    out_color = o.color; out_radii = o.radii;
  } else {
  cfg.flags |= GSR_FLAG_BACKWARD_FOLLOWS;  // the forward zero-fills the backward's accumulator rows on its way
  const Tensor means = f32c(means3d.unsqueeze(0)), cov = f32c(cov3d.reshape({n, 6}).unsqueeze(0)), opac = f32c(opacities.reshape({n}).unsqueeze(0));
  const Tensor colors = f32c(col_in.unsqueeze(0));
  c10::optional<Tensor> m2;
  if (means2d.has_value() && means2d->defined()) m2 = means2d->unsqueeze(0);
  ForwardOut r = rasterize_impl(pb, means, cov, opac, colors, c10::nullopt, m2, viewbuf, cfg, c10::nullopt, 1);
  out_color = r.color.select(0, 0); out_radii = r.radii.select(0, 0);
  }
  }
  return pybind11::make_tuple(out_color, out_radii);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "torch-facing binding of libgsr_hip.so (include/gsr.h): compiled autograd function, status policy, camera set-up";
  m.def("init", &init, "dlopen the raster library and resolve the C ABI");
  pybind11::list fields;
  for (const CfgField& f : kCfgFields) fields.append(f.name);
  m.attr("CFG_FIELDS") = pybind11::tuple(fields);  // RasterConfig's fields, in order, as this file states them
  m.def("launch_dims", [](const Cfg& cfg, int64_t capacity) { return cfg.launch_dims(capacity); }, "the GsrDims a launch of this call shape takes");
  m.def("call_shape", [](const Cfg& cfg) { return cfg; }, "the RasterConfig of any object with its fields (through Cfg and back)");
  pybind11::class_<PyBackend>(m, "Backend")
      .def(pybind11::init<>())
      .def_property("sync_policy", [](PyBackend& b) { return b.be().sync_policy == Backend::SyncPolicy::lazy ? "lazy" : "sync"; },
                    [](PyBackend& b, const std::string& v) {
                      if (v != "sync" && v != "lazy") throw pybind11::value_error("sync_policy must be 'sync' or 'lazy'");
                      b.be().sync_policy = v == "lazy" ? Backend::SyncPolicy::lazy : Backend::SyncPolicy::sync;
                    })
      .def_property("defer_after", [](PyBackend& b) { return b.be().defer_after.load(); }, [](PyBackend& b, int v) { b.be().defer_after = v; })
      .def_property("on_overflow", [](PyBackend& b) { return b.be().on_overflow == Backend::OnOverflow::nan ? "nan" : "raise"; },
                    [](PyBackend& b, const std::string& v) {
                      if (v != "nan" && v != "raise") throw pybind11::value_error("on_overflow must be 'nan' or 'raise'");
                      b.be().on_overflow = v == "nan" ? Backend::OnOverflow::nan : Backend::OnOverflow::raise;
                    })
      .def_property("defer_status", [](PyBackend& b) { return b.be().defer_status.load(); }, [](PyBackend& b, bool v) { b.be().defer_status = v; })
      .def_property("spin_us", [](PyBackend& b) { return b.be().spin_us.load(); }, [](PyBackend& b, double v) { b.be().spin_us = v; })
      .def_property("headroom_min", [](PyBackend& b) { return b.be().headroom_min.load(); }, [](PyBackend& b, double v) { b.be().headroom_min = std::max(1.0, v); })
      .def_property("headroom_max", [](PyBackend& b) { return b.be().headroom_max.load(); }, [](PyBackend& b, double v) { b.be().headroom_max = std::max(1.0, v); })
      .def_property("headroom_sigmas", [](PyBackend& b) { return b.be().headroom_sigmas.load(); }, [](PyBackend& b, double v) { b.be().headroom_sigmas = std::max(0.0, v); })
      .def("headroom_for", [](PyBackend& b, const ShapeKey& k) { return b.be().headroom_for(k); })
      .def_property_readonly("capacity_hint", [](PyBackend& b) { return b.be().capacity_hint(); })
      .def_property_readonly("seen", [](PyBackend& b) { return b.be().seen(); })
      .def_property_readonly("pending", [](PyBackend& b) { return b.be().pending_tokens(); })
      .def_property_readonly("poisoned", [](PyBackend& b) { return b.be().poisoned_tokens(); })
      .def_property_readonly("last_status", [](PyBackend& b) -> pybind11::object { return b.be().has_status() ? pybind11::object(status_dict(b.be().last_status())) : pybind11::none(); })
      .def_property_readonly("workspace_cache_size", [](PyBackend& b) { return b.be().workspace_cache_size(); })
      .def("set_capacity_hint", [](PyBackend& b, const ShapeKey& k, int64_t v) { b.be().set_capacity_hint(k, v); })
      .def("capacity_for", [](PyBackend& b, const Cfg& cfg, int64_t num_pairs, int max_list, double headroom) {
             Status st; st.num_pairs = num_pairs; st.max_list = max_list;
             return b.be().capacity_for(cfg, st, headroom);
           }, pybind11::arg("cfg"), pybind11::arg("num_pairs"), pybind11::arg("max_list"), pybind11::arg("headroom") = 1.25)
      .def("read_status", [](PyBackend& b, const Tensor& bin) {
             Status st;
             {
               pybind11::gil_scoped_release nogil;
               st = b.be().read_status(bin);
             }
             return status_dict(st);
           })
      .def("make_plan", [](PyBackend& b, const Cfg& cfg, const at::Device& device, int64_t capacity) {
             // the plan API's outputs and workspaces: (dims, color, extra_img | None, radii, geom, bin, img, backward-scratch bytes, alpha_img | None)
             const Plan p = b.be().make_plan(cfg, device, capacity, false);
             return pybind11::make_tuple(p.dims, p.color, or_none(p.extra_img), p.radii, p.geom, p.bin, p.img, b.be().sized(cfg, capacity).scratch,
                                         or_none(p.alpha_img));
           })
      .def("check_pending", [](PyBackend& b, bool wait, int64_t only_token) { pybind11::gil_scoped_release nogil; b.be().check_pending(wait, only_token); },
           pybind11::arg("wait") = false,
           pybind11::arg("only_token") = -1)
      .def("release_workspaces", [](PyBackend& b) { pybind11::gil_scoped_release nogil; b.be().release_workspaces(); })
      .def("forward", [](PyBackend& b, const Cfg& cfg, const Tensor& viewbuf, const Tensor& means, const Tensor& cov, const Tensor& opac,
                         const Tensor& colors, const c10::optional<Tensor>& extra, const c10::optional<Tensor>& frames, int64_t capacity, bool reuse_workspaces) {
             ForwardOut o;
             {
               pybind11::gil_scoped_release nogil;
               o = b.be().forward(cfg, viewbuf, means, cov, opac, colors, extra.has_value() ? *extra : Tensor(), frames.has_value() ? *frames : Tensor(),
                                  capacity, reuse_workspaces);
             }
             pybind11::object saved = pybind11::none();
             if (o.saved.valid) saved = pybind11::make_tuple(o.saved.dims, o.saved.geom, o.saved.bin, o.saved.img, o.saved.token);
             return pybind11::make_tuple(o.color, or_none(o.extra_img), o.radii, saved, or_none(o.alpha_img));
           }, pybind11::arg("cfg"), pybind11::arg("viewbuf"), pybind11::arg("means"), pybind11::arg("cov"), pybind11::arg("opac"), pybind11::arg("colors"),
           pybind11::arg("extra"), pybind11::arg("frames"), pybind11::arg("capacity") = -1, pybind11::arg("reuse_workspaces") = false)
      .def("backward", [](PyBackend& b, const Cfg& cfg, const GsrDims& dims, const Tensor& geom, const Tensor& bin, const Tensor& img,
                          int64_t token, const Tensor& viewbuf, const Tensor& means, const Tensor& cov, const Tensor& opac, const Tensor& colors,
                          const c10::optional<Tensor>& extra, const Tensor& g_color, const c10::optional<Tensor>& g_extra, bool want_means2d, bool rows_in_workspace,
                          const c10::optional<Tensor>& frames, int want_views, const c10::optional<Tensor>& g_alpha) {
             const Saved ws{true, dims, geom, bin, img, token};
             std::vector<Tensor> g;
             {
               pybind11::gil_scoped_release nogil;
               g = b.be().backward(cfg, ws, viewbuf, means, cov, opac, colors, extra.has_value() ? *extra : Tensor(), g_color,
                                   g_extra.has_value() ? *g_extra : Tensor(), want_means2d, rows_in_workspace, frames.has_value() ? *frames : Tensor(), want_views,
                                   g_alpha.has_value() ? *g_alpha : Tensor());
             }
             pybind11::list out;
             for (size_t k = 0; k < (want_views ? 7u : 6u); ++k) out.append(g[k].defined() ? pybind11::cast(g[k]) : pybind11::none());
             return pybind11::tuple(out);
           }, pybind11::arg("cfg"), pybind11::arg("dims"), pybind11::arg("geom"), pybind11::arg("bin"), pybind11::arg("img"), pybind11::arg("token"),
           pybind11::arg("viewbuf"), pybind11::arg("means"), pybind11::arg("cov"), pybind11::arg("opac"), pybind11::arg("colors"), pybind11::arg("extra"),
           pybind11::arg("g_color"), pybind11::arg("g_extra"), pybind11::arg("want_means2d"), pybind11::arg("rows_in_workspace"), pybind11::arg("frames"),
           pybind11::arg("want_views"), pybind11::arg("g_alpha") = pybind11::none());
  m.def("rasterize", &rasterize, pybind11::arg("backend"), pybind11::arg("means"), pybind11::arg("cov"), pybind11::arg("opac"), pybind11::arg("colors"),
        pybind11::arg("extra"), pybind11::arg("means2d"), pybind11::arg("viewbuf"), pybind11::arg("cfg"), pybind11::arg("frames"), pybind11::arg("camera_gradient"));
  m.def("rasterize_views", &rasterize_views);
  m.def("prepare_call", [](const Tensor& means, const Tensor& cov, const Tensor& opac, const Tensor& colors, const Tensor& viewbuf, int64_t h, int64_t w, int64_t sh_degree,
                           bool use_sh, int64_t views_per_set, const c10::optional<Tensor>& extra, const c10::optional<Tensor>& means2d, int64_t max_sh_eval,
                           bool sh_planar, bool cov_3x3, int64_t extra_mode, bool debug, bool prefiltered, int64_t deterministic, bool scale_rot,
                           const c10::optional<Tensor>& frames, int64_t camera_gradient, int64_t sh_frame) {
    const Prepared p = prepare_call(means, cov, opac, colors, viewbuf, h, w, sh_degree, use_sh, views_per_set, extra, means2d, max_sh_eval, sh_planar, cov_3x3,
                                    extra_mode, debug, prefiltered, deterministic, scale_rot, frames, camera_gradient, sh_frame);
    return pybind11::make_tuple(p.cfg, p.means, p.cov, p.opac, p.colors, p.extra, p.frames, p.viewbuf);  // (an optional without a value: None)
  }, "the call shape of rasterize_views (checks, normalisation, flags) without the operator: what any backend object runs behind");
  m.def("rasterize_one_view", &rasterize_one_view);
  m.def("views_from_cameras", &views_from_cameras);
  m.def("setup_views", &setup_views_raw);
  m.def("setup_views_backward", &setup_views_backward);
  m.def("setup_views_backward_ex", [](const Tensor& viewbuf, const Tensor& intrinsics, const Tensor& d_views, bool want_ext, bool want_intr) {
    const auto r = setup_views_backward_ex(viewbuf, intrinsics, d_views, want_ext, want_intr);
    return pybind11::make_tuple(or_none(std::get<0>(r)), or_none(std::get<1>(r)));
  });
  m.def("setup_views_orthographic", &setup_views_orthographic);
  m.def("mark_visible", &mark_visible);
  m.def("adapt", &adapt, "Gaussian adapter, one launch each way: (means (G, P, 3), scale + quaternion records (G, P, 7), masked harmonics (G, P, 3, M))");
  m.def("cov_from_scale_rot", &cov_from_scale_rot);
  m.def("cov_from_scale_rot_backward", &cov_from_scale_rot_backward);
  m.def("frames_arg", [](const Cfg& cfg, const c10::optional<Tensor>& frames) {
    // -> (frames as the launches take them | None, F): the frames check of the ctypes launches of the plan API
    const Tensor fr = frames_arg(cfg, frames.has_value() ? *frames : Tensor());
    return fr.defined() ? pybind11::make_tuple(fr, fr.size(1)) : pybind11::make_tuple(pybind11::none(), 0);
  });
  m.def("pack_view", [](const Tensor& vm, const Tensor& pm, const Tensor& cp, const Tensor& bg, double tx, double ty, const c10::optional<Tensor>& txt,
                        const c10::optional<Tensor>& tyt, double scale_modifier, const at::Device& device) {
    return pack_view(vm, pm, cp, bg, tx, ty, txt.has_value() ? *txt : Tensor(), tyt.has_value() ? *tyt : Tensor(), scale_modifier, device);
  });
}
