// libtsba.so -- MI355X (gfx950) bundle adjustment / pose optimisation for TextSLAM's optimizer:: hot path.
// C ABI in include/tsba.h.  One translation unit: kernels + Levenberg-Marquardt driver + ABI.
//
// Kernel sequence of one LM iteration (all launched back-to-back on one stream, no host sync; the LM state machine
// lives in device memory and every kernel starts by reading it):
//   k_schur   one wave per 6x6 block of the reduced camera system S (gather over landmark slot pairs) + reduced gradient
//   k_solve   one workgroup: blocked Cholesky of S in LDS, pose step
//   k_back    landmark back-substitution, candidate parameters x (+) dx, step norm, model cost change
//   k_linearize<COST>  candidate cost (residuals + Huber only)
//   k_decide  step quality, trust-region update, accept / reject, convergence tests (Ceres 1.x semantics)
//   k_linearize<FULL>  (only after an accepted step) residual + analytic Jacobian + IRLS weight + per-pair / per-group
//                      J^T J, J^T r, J^T J_landmark sums: one wave per (target KF, host KF) pair of scene observations,
//                      one wave per (KF, text) observation of up to 64 photometric blocks
//   k_mid     per landmark V, b and the host-pose column of W; per pair the host-side products
//   k_postlin pose diagonal / gradient, Jacobi scaling, cost, gradient tolerance
// Windows on one GPU (at most SCHUR_KEEP_KF keyframes) run a trial as FOUR launches: k_schur_t<4> (assembly; one more workgroup takes the full decision on the
// previous trial: new state, poses' rows, trace) | k_solve_back (solver + back-substitution) | k_linearize at the candidate | k_mid (+ its decision block: the light
// decision on this trial -- accept / reject, radius, current linearisation -- left in W.dec for the next k_schur_t<4>); a pass's last trial is decided by one workgroup of k_pass_end (k_decide's body; k_decide as a launch on every other path).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <chrono>
#include <thread>
#include <mutex>
#include <map>
#include <condition_variable>
#include <atomic>
#include <functional>
#include <dlfcn.h>
#include <rccl/rccl.h>      // types only: the library is dlopen()ed by tsba_comm_init, single-GPU use never touches RCCL
#include "../../include/tsba.h"
#include "../../include/tsba_debug.h"
#include "tsba_device.h"
#include "tsraster.h"
#include "tsquadstat.h"
#include "tsstage.h"
#include "tsba_plan.h"

#include "tsba_types.h"
#include "tsba_kernels_lin.h"
#include "tsba_kernels_schur.h"
#include "tsba_solve.h"
#include "tsba_solve_la.h"
#include "tsba_chol.h"
#include "tsba_band.h"
#include "tsba_bandp.h"
#include "tsba_bandcr.h"
#include "tsba_bandcre.h"
#include "tsba_bandms.h"
#include "tsba_bandsv.h"
#include "tsba_bandmx.h"
#include "tsba_layout.h"
#include "tsba_pcg.h"
#include "tsba_wb.h"
#include "tsba_pose.h"
#include "tsba_theta.h"

#include "tsba_kernels_step.h"
#include "tsba_kernels_pass.h"
#include "tsba_devplan.h"
// ---- LDS hygiene (tests): what a kernel finds in LDS is whatever the last workgroup on that compute unit left -- its own context's kernels when the device is
// otherwise idle (the same bytes every run: a read of never-written LDS goes unnoticed), another context's next to it (TextSLAM extracts ORB features while
// a bundle adjustment runs).  tsba_debug_options.lds_poison = 1 / 2 / 3 fills the LDS of every compute unit with NaNs / 1e300 / 0x5a bytes before EVERY launch
// of a solve: a kernel that reads what it has not written shows up as a changed result (tests/test_gpu_polling.py).
__global__ __launch_bounds__(256) void k_lds_poison(int pattern, int ndbl) {
    extern __shared__ __attribute__((aligned(16))) double pz[];
    const double v = pattern == 1 ? __longlong_as_double(0x7ff8000000000000LL) : pattern == 2 ? 1e300 : __longlong_as_double(0x5a5a5a5a5a5a5a5aLL);
    for (int k = threadIdx.x; k < ndbl; k += 256) pz[k] = v;
    __syncthreads();
    for (int k = 0; k < 40; k++) __builtin_amdgcn_s_sleep(127);      // (~2 us: long enough for every compute unit to be handed one of the workgroups)
}
static thread_local int g_lds_poison = 0;
static void lds_poison_hook(hipStream_t st) {
    if (!g_lds_poison) return;
    static std::once_flag once; std::call_once(once, [] { hipFuncSetAttribute((const void *)k_lds_poison, hipFuncAttributeMaxDynamicSharedMemorySize, 160*1024 - 256); });
    hipLaunchKernelGGL(k_lds_poison, dim3(1024), dim3(256), 160*1024 - 256, st, g_lds_poison, (160*1024 - 256)/8);
}
#define LAUNCHK(kern, grid, block, lds, st, ...) do { lds_poison_hook(st); hipLaunchKernelGGL(kern, grid, block, lds, st, __VA_ARGS__); } while (0)
// ------------------------------------------------------------------------------------------------ host side
static inline bool image_dims_ok(int w, int h) { return w > 0 && h > 0 && w <= TSBA_MAX_IMAGE_DIM && h <= TSBA_MAX_IMAGE_DIM; }
static int pose_grid(const LevelDev &D) { return std::max(1, (D.n_sc + 255)/256 + (D.n_pf + 31)/32); }    // workgroups of k_pose_iter
struct Ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool uploaded = false;
    tsba_options opt;
    int n_kf = 0, n_pt = 0, n_text = 0, n_tobs = 0, n_sgood = 0, n_tfgood = 0, n_levels = 0;
    Work W;
    std::vector<HostPlan> hplan;                  // per level (only levels used by the options are built)
    std::vector<LevelDev> lev;
    std::vector<int> lev_built;                   // level l is on the device (plan lists, reference features, image table)
    // one-shot calls on small windows stage a level when its pass begins (the coarse passes run while the plan of level 0 is still being built)
    std::vector<std::thread> planners;            // planners[l]: the host thread that builds level l's plan (joined by stage_level)
    std::vector<int> lev_planned;                 // a plan of level l was started for this upload
    const tsba_problem *stage_p = nullptr;        // the caller's problem while levels may still be staged from it (one-shot calls only)
    std::vector<int> ic_slot; bool use_img_cache = false;      // plane cache: slot of every keyframe of this upload
    std::atomic<int> plan_done[TSBA_MAX_LEVELS];  // set by a plan thread when its plan is complete: a level is staged ahead of its pass only when that costs no wait
    hipStream_t copy_stream = nullptr; hipEvent_t ev_stage[TSBA_MAX_LEVELS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_upload = nullptr; bool upload_pending = false;      // one-shot calls end their upload without a synchronisation: the copy stream's first staging waits for this event (the slabs' clearing runs on the compute stream)
    bool stage_async = false; int lev_wait[TSBA_MAX_LEVELS] = {0, 0, 0, 0};     // levels staged during a solve go over the copy stream; their pass waits for the event
    // restart copies
    double *pose0 = nullptr, *rho0 = nullptr, *theta0 = nullptr; uint8_t *sgood0 = nullptr, *tobs_good0 = nullptr, *tfgood0 = nullptr;
    uint8_t *kf_initial = nullptr;
    LmState *st_host = nullptr;                   // pinned: per-pass snapshots
    LmState *st_log = nullptr;                    // device [MAX passes]
    int nb_back_max = 0;
    LmState *st_base = nullptr;                   // W.st / W.st_next are st_base and st_base + 1 in the order of the moment
    double *musig2[2] = {nullptr, nullptr}; int musig_sel = 0;      // mu / sigma of the text observations, two buffers: k_pass_end fills the next pass's while the outlier pass reads this one's
    int *ticket = nullptr;                        // k_pass_begin: arrival counter of its participation workgroups (zero between launches)
    unsigned long long *lin_ticket = nullptr, lin_base = 0;      // k_lin_mid: arrivals of its workgroups over all launches since the upload (device), the same count on the host
    size_t lds_limit = 0;
    int n_cu = 0;                                 // compute units of the device
    std::vector<std::pair<std::pair<const void *, size_t>, int>> occ_cache;      // (kernel, dynamic LDS) -> workgroups of it one compute unit holds
    std::vector<uint8_t *> img_dev[TSBA_MAX_LEVELS];
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // RCCL (global BA sharded over the GPUs of one node): one process per GPU, communicator created by tsba_comm_init
    bool pose_only = false;                       // one keyframe, every landmark frozen in its host: the fused pose-only LM kernel applies
    double *S_alloc = nullptr; size_t S_count = 0;
    SolverLayout lay{};                             // what choose_solver_layout (tsba_layout.h) decided for this upload; the fields below are its copies where the solvers read them
    int S_up = CH_NB;                               // band storage: columns stored right of the diagonal + 1
    bool S_stale = true;                            // band storage: entries of another pass may be left in S (cleared before the next assembly)
    double *S_xchg = nullptr; int xchg_wp = 0;      // multi-GPU, band storage: packed band rows for the exchange (k_band_pack)
    bool sep_cr = false;                  // separator system by cyclic reduction on the compact block pool (tsba_bandcr.h)
    int band_parts = 1; double *Lb = nullptr, *Tbuf = nullptr, *Bpart = nullptr, *Ssep = nullptr, *Lcol_sep = nullptr, *CRcontrib = nullptr, *CRfac = nullptr; int *CRgate = nullptr; int cre_epoch = 0; int nsep_ld = 0; Work Wsep;   // partitioned band solver (tsba_bandp.h)
    double *Lcol = nullptr; int band_stream = 0;  // streaming band solver (tsba_band.h): L by block column; 1 = every built level fits it     // storage behind W.S (dense or band)
    DeviceBlock lbl_dev; PinnedBlock lbl_host;   // text label image staging
    DeviceBlock lat_dev; PinnedBlock lat_host;   // tsba_text_label_at: queries and labels [kf | px | label], device and pinned
    unsigned long long *hprog = nullptr; unsigned int pass_seq = 0;   // pinned progress word written by k_postlin / k_decide
    std::vector<struct Slab> slabs; int cur_slab = 0;
    int run_slab = 0; size_t run_off = 0, run_len = 0;   // pending contiguous host-to-device range
    int cur_bw_rows = 1 << 30;                     // band bound of the level being solved (set by launch_pass_init)
    // device cache of keyframe pyramid planes (tsba_problem.kf_id): one slot per keyframe, all levels of a keyframe contiguous
    struct ImgCache { uint8_t *dev = nullptr; PinnedBlock stage; size_t slot = 0, lvl_off[TSBA_MAX_LEVELS] = {0,0,0,0};
                      int w[TSBA_MAX_LEVELS] = {0,0,0,0}, h[TSBA_MAX_LEVELS] = {0,0,0,0}; unsigned lvl_mask = 0;
                      long long id[TSBA_IMG_CACHE_KF]; unsigned long long used[TSBA_IMG_CACHE_KF]; bool full[TSBA_IMG_CACHE_KF]; unsigned long long tick = 0;
                      long long hits = 0, misses = 0; } ic;
    WbBuf wb{}; Work Wk{}; DeviceBlock wb_alloc;      // low-rank correction for loop closures (tsba_wb.h): its buffers, the k x k dense system as a second Work
    EcgBuf ecg{}; DeviceBlock ecg_alloc;      // enlarged conjugate gradients (tsba_pcg.h)
    bool pack_in_solve = false, packed = false;   // one-shot calls: tsba_solve packs the results behind its last kernel (enqueue_pack); packed: the block in dl_host is that solve's
    DeviceBlock dl_dev; PinnedBlock dl_host;       // results of a solve as one block (k_pack_results): one device-to-host copy per download
    MsBuf sv{}; DeviceBlock sv_alloc; bool sv_prepared = false;      // single-vector solve phase (tsba_bandsv.h); sv_prepared: k_sv_linv has run on the current factorisation
    MsBuf ms{}; DeviceBlock ms_alloc; int ms_T = 0;      // multi-right-hand-side solve phase of the partitioned band solver (tsba_bandms.h)
    std::vector<int32_t> rb_r, rb_c; std::vector<double> rb_v;      // tsba_debug_reduced_blocks: the blocks between its two calls
    int cov_text = -1; double *cov_log = nullptr;     // tsba_theta_optim: V of this plane at the end of every pass [TSBA_MAX_LEVELS][6]
    // tsba_theta_optim_batch: an arena of its own (the resident problem of tsba_upload, its slabs and its plane cache are never touched).  dev = staged
    // block | scratch | output records; host = the pinned staging block (headers, frames, features, image planes); out = the pinned output records
    DeviceBlock tb_dev; PinnedBlock tb_host, tb_out;
    int far_B = 0, n_far = 0, pcg_parts = 0; unsigned int pcg_seq = 0;      // band + long-range blocks (tsba_pcg.h): band of M in pose blocks, blocks outside it, partial sums per vector kernel
    int rank = 0, world = 1; bool force_multi = false;
    tsba_debug_options dbg{};                      // test / diagnostics switches (tsba_debug_set), all zero in production
    struct LocalGroup *lgroup = nullptr;           // in-process communicator (tsba_comm_init_local)
    bool in_solve = false, has_token = false;      // local group: this rank is inside tsba_solve / holds the group's device token
    size_t x_acc = 0, x_trial = 0, x_lin = 0, x_pass = 0;   // bytes handed to collectives: running total; last LM trial / linearisation / pass set-up
    decltype(&ncclCommCount) p_count = nullptr;
    void *rccl_so = nullptr; ncclComm_t comm = nullptr;
    decltype(&ncclGetUniqueId) p_getid = nullptr; decltype(&ncclCommInitRank) p_init = nullptr;
    decltype(&ncclAllReduce) p_allreduce = nullptr; decltype(&ncclCommDestroy) p_destroy = nullptr;
    decltype(&ncclGetErrorString) p_errstr = nullptr;
};

static void set_err(Ctx *c, const std::string &s) { c->err = s; }
// Room for `need` bytes in one of the context's blocks that only grow (tsstage.h); where it must move it gets max(need, room) bytes, after a wait for the stream, which
// may still use the old one.  what names the block in the error text; nullptr where a failure only makes the caller take another path and nothing is reported.
template <class B> static int reserve(Ctx *c, B &b, const char *what, size_t need, size_t room = 0) {
    if (need <= b.cap()) return TSBA_OK;
    if (b.cap()) hipStreamSynchronize(c->stream);
    const hipError_t e = b.grow(need, room);
    if (e != hipSuccess && what) set_err(c, std::string(what) + ": " + hipGetErrorString(e));
    return e == hipSuccess ? TSBA_OK : TSBA_ERR_DEVICE;
}
// hipFuncAttributeMaxDynamicSharedMemorySize of a kernel, once per (kernel, device) and size class instead of before every solve (a global-BA solve made ~45 of these
// calls).  And with a retry: beside another host thread that was initialising an RCCL communicator the call has been seen to fail with "invalid device function" for a
// kernel it had accepted a thousand times (the runtime's function table while another library's code objects are being registered; the busy-context suite of round 6's
// final tree, profiles/r06_gpu_suite_beside_busy_contexts_final.txt) -- a transient of the runtime must not fail a solve.
static int set_attr_cached(Ctx *c, const void *fn, int bytes, const char *what) {
    static std::mutex mu; static std::map<std::pair<const void *, int>, int> granted;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(fn, c->device); const auto it = granted.find(key);
    if (it != granted.end() && it->second >= bytes) return 0;
    hipError_t e = hipSuccess;
    for (int t = 0; t < 6; t++) {
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess) break;
        (void)hipGetLastError(); std::this_thread::sleep_for(std::chrono::microseconds(100 << t));
    }
    if (e != hipSuccess) { set_err(c, std::string("hipFuncSetAttribute(") + what + "): " + hipGetErrorString(e)); return TSBA_ERR_DEVICE; }
    granted[key] = bytes; return 0;
}
#define ATTR(fn, bytes) do { const int rc_ = set_attr_cached(c, (const void *)(fn), (int)(bytes), #fn); if (rc_) return rc_; } while (0)
static bool is_multi(const Ctx *c);
// Kernels whose workgroups wait for each other inside ONE launch (value polling: k_solve_back, k_sv_cre_tree, k_sv_tree_back, k_cre_back_tree) make progress
// only if every workgroup of the launch has a compute unit.  They are chosen only where the whole grid fits the device at once (occupancy of that kernel
// with its dynamic LDS x compute units); otherwise the launch-per-step path that they replaced runs.  Other work on the device (a second context's
// kernels) can only DELAY the dispatch of a workgroup -- it ends without waiting for anything here -- and a wait that outlasts the polling bound is counted
// (ts_poll_giveups -> tsba_report.poll_timeouts) on top of failing the linear solve.
static bool grid_resident(Ctx *c, const void *fn, int threads, size_t lds, int grid) {
    int nb = -1;
    for (auto &e : c->occ_cache) if (e.first.first == fn && e.first.second == lds) nb = e.second;
    if (nb < 0) { if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, lds) != hipSuccess) nb = 0;
        c->occ_cache.push_back({{fn, lds}, nb}); }
    return (long long)nb*(c->dbg.assume_cus > 0 ? c->dbg.assume_cus : c->n_cu) >= grid;
}

// Device memory comes from a few large slabs (bump allocation, 256-byte aligned) that persist across uploads: the ~200 arrays
// of a problem cost no hipMalloc / hipFree / hipMemset each (one memset per slab and upload), and host data is staged through a
// pinned mirror of the slab so that consecutive uploads leave as ONE host-to-device copy (a plan is ~50 arrays per level).
struct Slab { char *dev = nullptr, *host = nullptr; size_t size = 0, used = 0; };
static void flush_run(Ctx *c) {
    if (c->run_len) { Slab &sl = c->slabs[c->run_slab];
        hipMemcpyAsync(sl.dev + c->run_off, sl.host + c->run_off, c->run_len, hipMemcpyHostToDevice, c->stage_async && c->copy_stream ? c->copy_stream : c->stream); c->run_len = 0; }
}
static int slab_take(Ctx *c, size_t bytes, int *slab, size_t *off) {
    for (;;) {
        if (c->cur_slab < (int)c->slabs.size()) { Slab &sl = c->slabs[c->cur_slab];
            if (sl.size - sl.used >= bytes) { *slab = c->cur_slab; *off = sl.used; sl.used += bytes; return 0; }
            c->cur_slab++; continue; }
        Slab sl; sl.size = std::max<size_t>(bytes, (size_t)64 << 20);
        hipError_t e = hipMalloc((void **)&sl.dev, sl.size);
        if (e != hipSuccess) { set_err(c, std::string("hipMalloc: ") + hipGetErrorString(e)); return TSBA_ERR_DEVICE; }
        hipMemsetAsync(sl.dev, 0, sl.size, c->stream);
        if (c->stage_async) hipStreamSynchronize(c->stream);     // (a slab born during a solve: the copy stream must not overtake its clearing)
        c->slabs.push_back(sl);
    }
}
// A piece that receives no host data (an allocation, an empty list) right behind the pending run of staged bytes: when it is small the run goes on across it --
// zeros in the pinned mirror, which is what the slab's clearing left on the device -- instead of ending there.  Round 6 (rocprofv3 timeline of a one-shot
// tsba_pose_optim call): a single-frame plan has some thirty empty lists, each of them cut the run, and the call left as ~30 copies of a few hundred bytes
// (3 - 4 us of host time and 5 - 10 us of device time EACH, one after the other in front of the first kernel) instead of three.
#define RUN_BRIDGE ((size_t)32 << 10)
static void run_bridge(Ctx *c, int si, size_t off, size_t bytes) {
    Slab &sl = c->slabs[si];
    if (c->run_len && c->run_slab == si && c->run_off + c->run_len == off && bytes <= RUN_BRIDGE && sl.host) { memset(sl.host + off, 0, bytes); c->run_len += bytes; }
}
template <typename T>
static int dev_alloc(Ctx *c, T **out, size_t n) {
    const size_t bytes = (std::max<size_t>(n, 1)*sizeof(T) + 255) & ~(size_t)255;
    int si; size_t off; int rc = slab_take(c, bytes, &si, &off); if (rc) return rc;
    *out = (T *)(c->slabs[si].dev + off); run_bridge(c, si, off, bytes); return 0;
}
template <typename T>
static int dev_upload(Ctx *c, const T **out, const T *src, size_t n) {
    const size_t bytes = (std::max<size_t>(n, 1)*sizeof(T) + 255) & ~(size_t)255;
    int si; size_t off; int rc = slab_take(c, bytes, &si, &off); if (rc) return rc;
    Slab &sl = c->slabs[si];
    *out = (const T *)(sl.dev + off);
    if (!n || !src) { run_bridge(c, si, off, bytes); return 0; }
    if (!sl.host) { hipError_t e = hipHostMalloc((void **)&sl.host, sl.size, hipHostMallocDefault);
        if (e != hipSuccess) { set_err(c, std::string("hipHostMalloc: ") + hipGetErrorString(e)); return TSBA_ERR_DEVICE; } }
    if (c->run_len && (c->run_slab != si || c->run_off + c->run_len != off)) flush_run(c);
    if (!c->run_len) { c->run_slab = si; c->run_off = off; }
    memcpy(sl.host + off, src, n*sizeof(T));
    if (bytes > n*sizeof(T)) memset(sl.host + off + n*sizeof(T), 0, bytes - n*sizeof(T));
    c->run_len = off + bytes - c->run_off;
    return 0;
}
template <typename T>
static int dev_upload_or_zeros(Ctx *c, const T **out, const T *src, size_t n) {       // an optional array of the problem: zeros where the caller passes none
    std::vector<T> z; if (!src) { z.assign(n, T(0)); src = z.data(); }
    return dev_upload(c, out, src, n);
}
template <typename T>
static int dev_upload_vec(Ctx *c, const T **out, const std::vector<T> &v) { return dev_upload(c, out, v.data(), v.size()); }

static void join_planners(Ctx *c) { for (auto &t : c->planners) if (t.joinable()) t.join(); c->planners.clear(); }
static void free_problem(Ctx *c) {
    join_planners(c); c->stage_p = nullptr;
    hipStreamSynchronize(c->stream);
    if (c->copy_stream) hipStreamSynchronize(c->copy_stream);       // (a level staged ahead of a pass that a failed solve never reached: its copy reads the slabs' pinned mirror)
    for (int l = 0; l < TSBA_MAX_LEVELS; l++) c->lev_wait[l] = 0;
    // the slabs stay (tsba_destroy frees them): zero what the last problem used, restart the bump allocation
    for (Slab &sl : c->slabs) { if (sl.used) hipMemsetAsync(sl.dev, 0, sl.used, c->stream); sl.used = 0; }
    c->cur_slab = 0; c->run_len = 0;
    c->uploaded = false; c->lev.clear(); c->lev_built.clear();      // (the host plans keep their storage for the next upload: HostPlan::recycle)
    for (int l = 0; l < TSBA_MAX_LEVELS; l++) c->img_dev[l].clear();
}

extern "C" {

void tsba_default_options_local(tsba_options *o) {
    memset(o, 0, sizeof(*o));
    o->w_sx = o->w_sy = 1.0/1.2; o->w_t = 1.0/0.2;                  // optimizer.cc:1350-1351
    o->huber_scene = sqrt(5.991); o->huber_text = 3.0;              // :1369, :1454
    o->n_passes = 3;
    for (int i = 0; i < 3; i++) { o->levels[i] = 2 - i; o->its[i] = 10; o->chi2_mono[i] = 12.25; o->chi2_text[i] = i == 2 ? 0.95 : 0.5; }  // :282-289
    o->text_bad_ratio = 0.99; o->state = TSBA_STATE_LOCAL; o->outlier_scene = o->outlier_text = 1;
    o->use_text = 1; o->filter_good = 1; o->text_jacobian = 0;
    o->initial_radius = 1e4; o->max_radius = 1e16; o->min_radius = 1e-32; o->min_relative_decrease = 1e-3;
    o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
    o->min_diagonal = 1e-6; o->max_diagonal = 1e32; o->lm_shard = 0; o->lm_nshard = 1;
}
void tsba_default_options_pose(tsba_options *o) { tsba_default_options_local(o); o->state = TSBA_STATE_NOTREACHWIN; }
void tsba_default_options_global(tsba_options *o) {
    tsba_default_options_local(o);
    o->w_sx = o->w_sy = o->w_t = 1.0; o->n_passes = 1; o->levels[0] = 0; o->its[0] = 20; o->chi2_mono[0] = 18.0;   // :411-414
    o->state = TSBA_STATE_GLOBAL; o->outlier_scene = o->outlier_text = 0; o->use_text = 0; o->filter_good = 0;
}

void tsba_default_options_init(tsba_options *o) {                    // optimizer.cc:960-1056
    tsba_default_options_local(o);
    o->w_sx = o->w_sy = o->w_t = 1.0; o->huber_scene = 3.0; o->huber_text = 3.0;
    o->n_passes = 4; for (int i = 0; i < 4; i++) { o->levels[i] = 3 - i; o->its[i] = 10; }
    o->state = TSBA_STATE_NOTREACHWIN; o->outlier_scene = o->outlier_text = 0; o->filter_good = 0;
}
void tsba_default_options_landmarker(tsba_options *o) {              // optimizer.cc:531-541,1861,1873,1922
    tsba_default_options_local(o);
    o->w_sx = o->w_sy = o->w_t = 1.0; o->huber_scene = sqrt(5.991); o->huber_text = 2.0;
    o->n_passes = 4; for (int i = 0; i < 4; i++) { o->levels[i] = 3 - i; o->its[i] = 50; o->chi2_mono[i] = 18.0; o->chi2_text[i] = 1.5; }
    o->state = TSBA_STATE_NOTREACHWIN; o->outlier_scene = 1; o->outlier_text = 0;
}
void tsba_default_options_theta(tsba_options *o) {                   // optimizer.cc:610-615,2176,2203-2209
    tsba_default_options_local(o);
    o->w_sx = o->w_sy = o->w_t = 1.0; o->huber_text = 1e300;          // LossFunction* = nullptr
    for (int i = 0; i < 3; i++) o->its[i] = 50;
    o->state = TSBA_STATE_NOTREACHWIN; o->outlier_scene = o->outlier_text = 0; o->filter_good = 0;
}

int tsba_create(void **ctx, int device) {
    if (!ctx) return TSBA_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return TSBA_ERR_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return TSBA_ERR_DEVICE;
    Ctx *c = new Ctx(); c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return TSBA_ERR_DEVICE; }
    for (int l = 0; l < TSBA_MAX_LEVELS; l++) c->plan_done[l].store(0);
    if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) c->copy_stream = nullptr;     // (optional: staging then shares the compute stream)
    for (int l = 0; l < TSBA_MAX_LEVELS; l++) if (hipEventCreateWithFlags(&c->ev_stage[l], hipEventDisableTiming) != hipSuccess) c->ev_stage[l] = nullptr;
    if (hipEventCreateWithFlags(&c->ev_upload, hipEventDisableTiming) != hipSuccess) c->ev_upload = nullptr;
    hipDeviceProp_t prop;
    const bool ok = hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess
        && hipHostMalloc((void **)&c->st_host, sizeof(LmState)*TSBA_MAX_LEVELS + 64, 0) == hipSuccess
        && hipMalloc((void **)&c->st_log, sizeof(LmState)*TSBA_MAX_LEVELS) == hipSuccess
        && hipGetDeviceProperties(&prop, device) == hipSuccess;
    if (!ok) {                                      // nothing half-built leaves this function
        if (c->ev0) hipEventDestroy(c->ev0); if (c->ev1) hipEventDestroy(c->ev1);
        if (c->st_host) hipHostFree(c->st_host); if (c->st_log) hipFree(c->st_log);
        hipStreamDestroy(c->stream); delete c; return TSBA_ERR_DEVICE;
    }
    if (hipHostMalloc((void **)&c->hprog, 64, hipHostMallocDefault) != hipSuccess) c->hprog = nullptr; else memset(c->hprog, 0, 64);   // (optional: early-exit polling only)
    c->n_cu = prop.multiProcessorCount;
    c->lds_limit = prop.sharedMemPerBlock;       // 64 KiB default static limit; dynamic up to 160 KiB on gfx950
    if (c->lds_limit < 160*1024) c->lds_limit = 160*1024;
    *ctx = c; return TSBA_OK;
}
static void lgroup_forget(Ctx *c);              // (defined with LocalGroup below)
int tsba_destroy(void *ctx) {
    Ctx *c = (Ctx *)ctx; if (!c) return TSBA_ERR_ARG;
    hipSetDevice(c->device);
    lgroup_forget(c);
    free_problem(c);
    hipStreamSynchronize(c->stream); if (c->copy_stream) hipStreamSynchronize(c->copy_stream);
    for (Slab &sl : c->slabs) { hipFree(sl.dev); if (sl.host) hipHostFree(sl.host); }
    c->slabs.clear();
    if (c->comm && c->p_destroy) c->p_destroy(c->comm);
    hipHostFree(c->st_host); hipFree(c->st_log); if (c->hprog) hipHostFree(c->hprog);
    if (c->ic.dev) hipFree(c->ic.dev);
    for (int l = 0; l < TSBA_MAX_LEVELS; l++) if (c->ev_stage[l]) hipEventDestroy(c->ev_stage[l]);
    if (c->ev_upload) hipEventDestroy(c->ev_upload);
    if (c->copy_stream) hipStreamDestroy(c->copy_stream);
    hipEventDestroy(c->ev0); hipEventDestroy(c->ev1); hipStreamDestroy(c->stream);
    delete c; return TSBA_OK;                     // the blocks that only grow (tsstage.h) go with the context
}
int tsba_abi_version(void) { return TSBA_ABI_VERSION; }
const char *tsba_last_error(void *ctx) { return ctx ? ((Ctx *)ctx)->err.c_str() : "null ctx"; }

// the pyramid levels the passes use, each once, in the order of the first pass that uses it
static std::vector<int> levels_used(const tsba_options *o, int n_levels) {
    std::vector<int> used; std::vector<char> seen(n_levels, 0);
    for (int q = 0; q < o->n_passes; q++) if (!seen[o->levels[q]]) { seen[o->levels[q]] = 1; used.push_back(o->levels[q]); }
    return used;
}
// Every index the plan builder and the kernels dereference is range-checked here, once, in O(problem size): a bad index from the
// adapter becomes TSBA_ERR_ARG instead of a host out-of-bounds read or a GPU memory fault (the library never aborts the process).
static int check_problem(Ctx *c, const tsba_problem *p, const tsba_options *o) {
    auto bad = [&](const char *what) { set_err(c, std::string("invalid problem: ") + what); return TSBA_ERR_ARG; };
    if (!p || !o) return bad("null problem / options");
    if (p->n_kf <= 0 || p->n_levels < 1 || p->n_levels > TSBA_MAX_LEVELS) return bad("n_kf / n_levels");
    if (p->n_pt < 0 || p->n_text < 0 || p->n_tobs < 0 || p->n_sgood < 0) return bad("negative count");
    if (o->n_passes < 1 || o->n_passes > TSBA_MAX_LEVELS) return bad("n_passes");
    for (int i = 0; i < o->n_passes; i++) if (o->levels[i] < 0 || o->levels[i] >= p->n_levels) return bad("pass level out of range");
    if (o->text_jacobian != 0) { set_err(c, "text_jacobian=1 (numeric diff) is oracle-only"); return TSBA_ERR_ARG; }
    if (o->lm_nshard < 1 || o->lm_shard < 0 || o->lm_shard >= o->lm_nshard) return bad("lm_shard / lm_nshard");
    if (!p->pose) return bad("pose is null");
    if (p->n_pt > 0 && (!p->rho || !p->pt_ray || !p->pt_host)) return bad("null point array");
    if (p->n_text > 0 && (!p->theta || !p->text_host || !p->text_box_ray)) return bad("null text-plane array");
    if (p->n_sgood > 0 && !p->sgood) return bad("sgood is null");
    bool frozen = false;
    for (int j = 0; j < p->n_pt; j++) { const int h = p->pt_host[j]; if (h < -1 || h >= p->n_kf) return bad("pt_host out of range"); frozen |= h < 0; }
    if (frozen && !p->pt_host_Trw) return bad("pt_host_Trw is null but a point has a frozen host");
    frozen = false;
    for (int j = 0; j < p->n_text; j++) { const int h = p->text_host[j]; if (h < -1 || h >= p->n_kf) return bad("text_host out of range"); frozen |= h < 0; }
    if (frozen && !p->text_host_Twr) return bad("text_host_Twr is null but a plane has a frozen host");
    if (p->n_tobs > 0) {
        if (!p->tobs_kf || !p->tobs_text || !p->tobs_good || !p->tobs_fgood_off) return bad("null text-observation array");
        if (p->tobs_fgood_off[0] < 0) return bad("tobs_fgood_off[0] < 0");
        for (int t = 0; t < p->n_tobs; t++) {
            if (p->tobs_kf[t] < 0 || p->tobs_kf[t] >= p->n_kf) return bad("tobs_kf out of range");
            if (p->tobs_text[t] < 0 || p->tobs_text[t] >= p->n_text) return bad("tobs_text out of range");
            if (p->tobs_fgood_off[t+1] < p->tobs_fgood_off[t]) return bad("tobs_fgood_off not monotone");
        }
        if (p->tobs_fgood_off[p->n_tobs] > 0 && !p->tfgood) return bad("tfgood is null");
    }
    std::vector<int32_t> maxraw;
    for (const int l : levels_used(o, p->n_levels)) {
        const int ns = p->n_sobs[l];
        if (ns < 0) return bad("n_sobs < 0");
        if (ns > 0) {
            if (!p->sobs_kf[l] || !p->sobs_pt[l] || !p->sobs_flag[l] || !p->sobs_uv0[l]) return bad("null scene-observation array");
            const int32_t *kf = p->sobs_kf[l], *pt = p->sobs_pt[l], *fl = p->sobs_flag[l];
            for (int s = 0; s < ns; s++) {
                if ((unsigned)kf[s] >= (unsigned)p->n_kf) return bad("sobs_kf out of range");
                if ((unsigned)pt[s] >= (unsigned)p->n_pt) return bad("sobs_pt out of range");
                if ((unsigned)fl[s] >= (unsigned)p->n_sgood) return bad("sobs_flag out of range");
            }
        }
        if (p->n_text > 0 && p->tfeat_off[l]) {             // (a level without text features passes tfeat_off = NULL)
            const int32_t *off = p->tfeat_off[l]; const int nf = p->n_tfeat[l];
            if (nf < 0 || off[0] < 0 || off[p->n_text] > nf) return bad("tfeat_off out of range");
            for (int j = 0; j < p->n_text; j++) if (off[j+1] < off[j]) return bad("tfeat_off not monotone");
            if (off[p->n_text] > off[0] && (!p->tfeat_raw[l] || !p->tfeat_uv[l] || !p->tfeat_ref[l])) return bad("null text-feature array");
            maxraw.assign(p->n_text, -1);                  // a feature's flag is tfgood[tobs_fgood_off[t] + raw]: raw must fit every observation's span
            for (int j = 0; j < p->n_text; j++) for (int f = off[j]; f < off[j+1]; f++) {
                const int r = p->tfeat_raw[l][f]; if (r < 0) return bad("tfeat_raw < 0"); maxraw[j] = std::max(maxraw[j], (int32_t)r); }
            for (int t = 0; t < p->n_tobs; t++)
                if (maxraw[p->tobs_text[t]] >= p->tobs_fgood_off[t+1] - p->tobs_fgood_off[t]) return bad("tfeat_raw exceeds the observation's flag span");
        }
        if (o->use_text && p->n_tobs > 0)
            if (!p->img[l] || !image_dims_ok(p->img_w[l], p->img_h[l])) { set_err(c, "missing image level or image side above TSBA_MAX_IMAGE_DIM (" + std::to_string(TSBA_MAX_IMAGE_DIM) + ")"); return TSBA_ERR_ARG; }
    }
    return 0;
}

static int stage_level(Ctx *c, const tsba_problem *p, int l, double *t_plan, double *t_img);
// ---- the upload, stage by stage: upload_impl at the end is the list of calls, and every stage says what it leaves behind.  The slabs are bump allocators and
// dev_upload joins consecutive staged ranges into one host-to-device copy: the ORDER of the dev_upload / dev_alloc calls across the stages, sizes included, is
// part of the behaviour -- it fixes every buffer's address and the number of copies in front of the first kernel.
#define UP(dst, src, n) do { const int rc_ = dev_upload(c, &(dst), (src), (size_t)(n)); if (rc_) return rc_; } while (0)
#define UPZ(dst, src, n) do { const int rc_ = dev_upload_or_zeros(c, &(dst), (src), (size_t)(n)); if (rc_) return rc_; } while (0)
#define AL(dst, n) do { const int rc_ = dev_alloc(c, &(dst), (size_t)(n)); if (rc_) return rc_; } while (0)
typedef std::chrono::steady_clock UpClock;
static double ms_between(UpClock::time_point a, UpClock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
struct UploadTimes { UpClock::time_point t0, t1; double plan = 0.0, img = 0.0; bool verbose = false; };      // tsba_debug_options.verbose: the timing line
struct PlannerJoiner { Ctx *c; bool armed; ~PlannerJoiner() { if (armed) join_planners(c); } };             // on the error returns
struct PlanStart { bool defer = false, single_frame = false; std::function<void()> first_plan; };          // first_plan: a deferring call's first level, built on the calling thread
// sizes of the buffers that every level shares: what the levels on the device hold, what a level staged later can hold at most
struct LevelMax { size_t pair = 1, tg = 1, pslot = 1, tslot = 1, cnt = 1, pose_grid = 1;
    void take(const LevelMax &m) { pair = std::max(pair, m.pair); tg = std::max(tg, m.tg); pslot = std::max(pslot, m.pslot); tslot = std::max(tslot, m.tslot);
                                   cnt = std::max(cnt, m.cnt); pose_grid = std::max(pose_grid, m.pose_grid); } };
static LevelMax level_size(const LevelDev &D) {
    LevelMax m; m.pair = (size_t)D.n_pair; m.tg = (size_t)D.n_tg; m.pslot = (size_t)D.n_pslot; m.tslot = (size_t)D.n_tslot; m.cnt = (size_t)D.n_sc + D.n_tg; m.pose_grid = (size_t)pose_grid(D);
    return m;
}
static LevelMax level_capacity(const tsba_problem *p, int l) {
    const size_t nsc = (size_t)p->n_sobs[l], ntg = (size_t)p->n_tobs; size_t npf = 0;
    if (p->tfeat_off[l]) for (int q = 0; q < p->n_tobs; q++) { const int j = p->tobs_text[q]; npf += (size_t)(p->tfeat_off[l][j + 1] - p->tfeat_off[l][j]); }
    LevelMax m; m.pair = std::min((size_t)p->n_kf*((size_t)p->n_kf + 1), nsc + ntg); m.tg = ntg; m.pslot = nsc + (size_t)p->n_pt; m.tslot = ntg + (size_t)p->n_text; m.cnt = nsc + ntg;
    m.pose_grid = (nsc + 255)/256 + (npf + 31)/32 + 1;
    return m;
}
static int max_band_rows(const Ctx *c) { int bw = 0; for (int l = 0; l < c->n_levels; l++) if (c->lev_built[l]) bw = std::max(bw, c->lev[l].bw_rows); return bw; }

// leaves the context's copy of the options (returned; a rank's shard set), the counts and the scalars of Work
static const tsba_options *begin_upload(Ctx *c, const tsba_problem *p, const tsba_options *o) {
    c->opt = *o;
    if (c->world > 1) { c->opt.lm_shard = c->rank; c->opt.lm_nshard = c->world; }
    o = &c->opt;
    c->n_kf = p->n_kf; c->n_pt = p->n_pt; c->n_text = p->n_text; c->n_tobs = p->n_tobs; c->n_sgood = p->n_sgood; c->n_levels = p->n_levels;
    c->n_tfgood = p->n_tobs > 0 ? p->tobs_fgood_off[p->n_tobs] : 0;
    c->nb_back_max = back_blocks_pt(p->n_pt) + back_blocks_tx(p->n_text) + (p->n_kf + 255)/256;      // k_back's blocks (at least k_mid's landmark blocks)
    Work &W = c->W; memset(&W, 0, sizeof(W));
    W.n_kf = p->n_kf; W.n_pt = p->n_pt; W.n_text = p->n_text; W.n_tobs = p->n_tobs; W.N = 6*p->n_kf;
    for (int k = 0; k < 4; k++) W.K0[k] = p->K[k];
    W.w_sx = o->w_sx; W.w_sy = o->w_sy; W.w_t = o->w_t; W.huber_s = o->huber_scene; W.huber_t = o->huber_text;
    W.filter_good = o->filter_good; W.min_diag = o->min_diagonal; W.max_diag = o->max_diagonal;
    W.rank = c->rank; W.world = c->world;
    return o;
}
// leaves the plan of every level the passes use under way: on a host thread of its own, built already (single-frame problems), or as first_plan.
// The per-level plans are independent of each other and of the uploads that follow: one host thread per level builds them while the calling
// thread stages the parameter / observation arrays (C4: 1.6 ms of plan construction in sequence -> the largest level, overlapped)
static PlanStart start_plans(Ctx *c, const tsba_problem *p, const tsba_options *o, bool lazy, UploadTimes &T) {
    c->hplan.resize(p->n_levels); c->lev.resize(p->n_levels); c->lev_built.assign(p->n_levels, 0); c->lev_planned.assign(p->n_levels, 0);
    c->planners.clear(); c->planners.resize(p->n_levels);
    for (int l = 0; l < TSBA_MAX_LEVELS; l++) { c->plan_done[l].store(0); c->lev_wait[l] = 0; }
    const std::vector<int> used = levels_used(o, p->n_levels); const int n_lev = (int)used.size();
    PlanStart S;
    // (round 6: also the single-frame problems of tsba_pose_optim -- the plans of the later passes' levels are built and staged while the first pass runs)
    // (round 6: a single-frame problem with every landmark frozen -- tsba_pose_optim, per frame -- has a plan that is a copy of its input: written down directly
    // on this thread for every level (build_plan_single_frame, microseconds), no plan threads, every level staged before the solve)
    S.single_frame = plan_is_single_frame(p, o) && c->dbg.host_pair_lists != 1;
    S.defer = lazy && lds_solver_fits(c->W.N) && n_lev > 1 && !is_multi(c) && !S.single_frame;      // small windows only
    const auto tp0 = UpClock::now();
    const bool tdbg = T.verbose, reorder = !c->dbg.no_kf_reorder;
    // ring maps (one loop closure): a single-level, single-GPU solve through the partitioned solver with the cyclic-reduction separator tree
    const int ring_max = (n_lev == 1 && !c->dbg.no_ring && !c->dbg.no_band_stream && c->dbg.sep_solver != 1 && c->dbg.sep_solver != 3 && c->dbg.band_parts != 1) ? CR_SMAX/6 : 0;
    // maps with long-range coupling (several loop closures, points seen again much later): band + blocks outside it, preconditioned conjugate gradients
    const int far_max = (n_lev == 1 && c->dbg.far_solver != 1 && !c->dbg.no_band_stream && (!c->dbg.no_ring || c->dbg.far_solver >= 2)) ? CR_SMAX/6 : 0;     // (no_ring asks for the reordering path)
    const bool far_force = c->dbg.far_solver == 2 || c->dbg.far_solver == 3;
    // the point slot pairs by S block are built on the device (tsba_devplan.h) -- since round 4 on maps of more than 126 keyframes (2 M pairs: 9 of the plan's 21 ms), since round 6 on
    // windows as well: they are the largest part of a window's plan (C4 level 2: 0.18 of 0.5 ms on the calling thread of a one-shot call, level 0: 0.7 of 1.5 ms), the three small
    // launches that build them cost the pass ~15 us, the lists are the same entries in the same order (same bits: test_schur_lists_built_on_the_device_equal_the_host_lists)
    // (... on problems of at least 4096 scene observations: below, the three launches cost a level more than the host's lists -- InitBA's pair, a landmark's refinement, a plane's:
    // 15 us per level of calls that take 1.3 - 2.3 ms in launch-bound trials of ~32 us; tsba_debug_options.host_pair_lists = 2 asks for the device lists at any size)
    const bool dev_pairs = p->n_kf > 1 && c->dbg.host_pair_lists != 1 && (c->dbg.host_pair_lists == 2 || p->n_sobs[0] >= 4096);
    for (int i = n_lev - 1; i >= 0; i--) {         // (a level is started with the first pass that uses it)
        const int l = used[(size_t)i];
        HostPlan *H = &c->hplan[l];
        c->lev_planned[l] = 1;
        std::atomic<int> *done = &c->plan_done[l];
        // the levels of the later passes first (the largest plans); a deferring call builds the first pass's (small) plan on this thread:
        // it is needed at once, and a thread's start costs as much as that plan
        if (S.single_frame) { build_plan_single_frame(p, o, l, *H); done->store(1); continue; }
        if (S.defer && i == 0) { S.first_plan = [=]() { build_plan(p, o, l, *H, tdbg, reorder, ring_max, far_max, far_force, dev_pairs); done->store(1); }; continue; }    // (built by stage_levels, behind the problem arrays' copy)
        c->planners[l] = std::thread([p, o, l, H, tdbg, reorder, ring_max, far_max, far_force, dev_pairs, done]() { build_plan(p, o, l, *H, tdbg, reorder, ring_max, far_max, far_force, dev_pairs); done->store(1, std::memory_order_release); }); }
    T.plan += ms_between(tp0, UpClock::now());
    return S;
}
// leaves the parameters (and their restart copies), the landmark and observation arrays and the per-problem work arrays on the slabs
static int upload_problem_arrays(Ctx *c, const tsba_problem *p) {
    Work &W = c->W;
    const double *cd; const uint8_t *cu;
    UP(cd, p->pose, 7*(size_t)p->n_kf); c->pose0 = (double *)cd;
    UP(cd, p->rho, p->n_pt); c->rho0 = (double *)cd;
    UP(cd, p->theta, 3*(size_t)p->n_text); c->theta0 = (double *)cd;
    UP(cu, p->sgood, p->n_sgood); c->sgood0 = (uint8_t *)cu;
    UP(cu, p->tobs_good, p->n_tobs); c->tobs_good0 = (uint8_t *)cu;
    UP(cu, p->tfgood, c->n_tfgood); c->tfgood0 = (uint8_t *)cu;
    UPZ(cu, p->kf_initial, p->n_kf); c->kf_initial = (uint8_t *)cu;
    for (int b = 0; b < 2; b++) { AL(W.pose[b], 7*(size_t)p->n_kf); AL(W.rho[b], p->n_pt); AL(W.theta[b], 3*(size_t)p->n_text); }
    AL(W.sgood, p->n_sgood); AL(W.tobs_good, p->n_tobs); AL(W.tfgood, c->n_tfgood);
    UP(W.pt_ray, p->pt_ray, 2*(size_t)p->n_pt); UP(W.pt_host, p->pt_host, p->n_pt);
    UPZ(W.pt_Trw, p->pt_host_Trw, 12*(size_t)p->n_pt);
    UP(W.text_host, p->text_host, p->n_text);
    UPZ(W.text_Twr, p->text_host_Twr, 12*(size_t)p->n_text);
    UP(W.text_box, p->text_box_ray, 8*(size_t)p->n_text);
    UP(W.tobs_kf, p->tobs_kf, p->n_tobs); UP(W.tobs_text, p->tobs_text, p->n_tobs); UP(W.tobs_fgood_off, p->tobs_fgood_off, (size_t)p->n_tobs + 1);
    AL(c->musig2[0], 2*(size_t)p->n_tobs); AL(c->musig2[1], 2*(size_t)p->n_tobs); c->musig_sel = 0; W.musig = c->musig2[0];
    AL(c->ticket, 4); W.poll0 = (unsigned int *)(c->ticket + 1);
    AL(c->lin_ticket, 2); c->lin_base = 0;                         // (slab memory: zero)
    AL(W.kf_in, p->n_kf); AL(W.kf_const, p->n_kf); AL(W.act_pt, p->n_pt); AL(W.act_tx, p->n_text);
    AL(W.fidx, p->n_kf); AL(W.nfree, 2); AL(W.dbg, 64); AL(W.trace, 4*(size_t)TSBA_TRACE_CAP*TSBA_MAX_LEVELS); AL(W.LDbuf, 32*((size_t)p->n_kf + BAND_BW_MAX/6 + 1));     // (+ the ghost blocks of a ring map)
    return 0;
}
// plane cache (tsba_problem.kf_id): leaves every keyframe of this call with a slot (ic_slot); the planes of those not seen before are staged and copied.
// A failed call leaves no half state: no slot marked full without its planes
static int assign_plane_cache(Ctx *c, const tsba_problem *p, const tsba_options *o) {
    std::vector<int> &ic_slot = c->ic_slot; ic_slot.clear();
    c->use_img_cache = false;
    if (!(p->kf_id && !o->img_on_device && o->use_text && p->n_tobs > 0 && p->n_kf <= TSBA_IMG_CACHE_KF)) return 0;
    Ctx::ImgCache &IC = c->ic;
    unsigned mask = 0; size_t off = 0, lo[TSBA_MAX_LEVELS] = {0,0,0,0}; bool same = IC.dev != nullptr;
    for (int l : levels_used(o, p->n_levels)) if (p->img[l]) mask |= 1u << l;
    for (int l = 0; l < p->n_levels; l++) if (mask >> l & 1) { lo[l] = off; off += ((size_t)p->img_w[l]*p->img_h[l] + 255) & ~(size_t)255;
        same = same && IC.w[l] == p->img_w[l] && IC.h[l] == p->img_h[l]; }
    same = same && IC.lvl_mask == mask && IC.slot == off;
    if (!mask || !off) return 0;
    if (!same) {                                     // new geometry (or first use): an empty cache of TSBA_IMG_CACHE_KF slots
        hipStreamSynchronize(c->stream);
        if (IC.dev) { hipFree(IC.dev); IC.dev = nullptr; }
        if (hipMalloc((void **)&IC.dev, off*TSBA_IMG_CACHE_KF) != hipSuccess) { IC.dev = nullptr; set_err(c, "hipMalloc (plane cache)"); return TSBA_ERR_DEVICE; }
        IC.slot = off; IC.lvl_mask = mask;
        for (int l = 0; l < TSBA_MAX_LEVELS; l++) { IC.lvl_off[l] = lo[l]; IC.w[l] = l < p->n_levels ? p->img_w[l] : 0; IC.h[l] = l < p->n_levels ? p->img_h[l] : 0; }
        for (int q = 0; q < TSBA_IMG_CACHE_KF; q++) { IC.id[q] = 0; IC.used[q] = 0; IC.full[q] = false; }
    }
    for (int l = 0; l < p->n_levels; l++) if (mask >> l & 1) for (int k = 0; k < p->n_kf; k++)      // before any slot changes hands: a failed call must not leave a slot marked full without its planes
        if (!p->img[l][k]) { set_err(c, "null image pointer"); return TSBA_ERR_ARG; }
    IC.tick++;
    ic_slot.assign((size_t)p->n_kf, -1);
    std::vector<int> miss;
    for (int k = 0; k < p->n_kf; k++) { for (int q = 0; q < TSBA_IMG_CACHE_KF; q++) if (IC.full[q] && IC.id[q] == p->kf_id[k]) { ic_slot[(size_t)k] = q; IC.used[q] = IC.tick; break; }
        if (ic_slot[(size_t)k] < 0) miss.push_back(k); }
    for (int k : miss) { int best = -1;              // least recently used slot that this call does not use
        for (int q = 0; q < TSBA_IMG_CACHE_KF; q++) if (IC.used[q] != IC.tick && (best < 0 || !IC.full[q] || (IC.full[best] && IC.used[q] < IC.used[best]))) { best = q; if (!IC.full[q]) break; }
        IC.id[best] = p->kf_id[k]; IC.full[best] = true; IC.used[best] = IC.tick; ic_slot[(size_t)k] = best; }
    IC.hits += p->n_kf - (long long)miss.size(); IC.misses += (long long)miss.size();
    if (!miss.empty()) {
        const size_t need = miss.size()*off;
        if (int rc = reserve(c, IC.stage, "plane cache staging", need)) {
            for (int k : miss) IC.full[ic_slot[(size_t)k]] = false;          // (their planes were never copied)
            return rc; }
        uint8_t *stage = IC.stage.as<uint8_t>();
        for (size_t m = 0; m < miss.size(); m++) { const int k = miss[m];
            for (int l = 0; l < p->n_levels; l++) if (mask >> l & 1) memcpy(stage + m*off + lo[l], p->img[l][k], (size_t)p->img_w[l]*p->img_h[l]);
            hipMemcpyAsync(IC.dev + (size_t)ic_slot[(size_t)k]*off, stage + m*off, off, hipMemcpyHostToDevice, c->stream); }
    }
    c->use_img_cache = true;
    return 0;
}
// leaves on the device the levels the solve needs before it starts -- all of them, unless the call defers: then the first pass's only, the others are staged when
// their pass begins (stage_p) -- and in *mx what the buffers shared by all levels must hold
static int stage_levels(Ctx *c, const tsba_problem *p, const tsba_options *o, const PlanStart &S, LevelMax *mx, UploadTimes &T) {
    if (S.first_plan) {                              // a deferring call: the first pass's plan on this thread, while the problem arrays (and a new keyframe's planes) cross the bus
        flush_run(c);
        const auto tp0 = UpClock::now(); S.first_plan();
        T.plan += ms_between(tp0, UpClock::now()); }
    const std::vector<int> used = levels_used(o, p->n_levels);
    for (size_t i = 0; i < used.size(); i++) {
        const int l = used[i];
        if (S.defer && i > 0) { mx->take(level_capacity(p, l)); continue; }
        const int rc = stage_level(c, p, l, &T.plan, &T.img); if (rc) return rc;
        mx->take(level_size(c->lev[l]));
    }
    c->stage_p = S.defer ? p : nullptr;
    return 0;
}
// decides the fused pose-only path (one keyframe, every landmark frozen in its host) and leaves its state and per-workgroup partial sums
static int alloc_pose_buffers(Ctx *c, const tsba_problem *p, const LevelMax &mx) {
    Work &W = c->W;
    c->pose_only = p->n_kf == 1 && every_landmark_frozen(p) && !c->dbg.no_pose_kernel;
    W.pst = nullptr; W.ppart = nullptr;
    if (c->pose_only) { AL(W.pst, 2); AL(W.ppart, 3*28*mx.pose_grid); }
    return 0;
}
// leaves the two linearisation buffers (current / candidate) and the Jacobi scaling
static int alloc_lin_buffers(Ctx *c, const tsba_problem *p, const LevelMax &mx) {
    Work &W = c->W;
    for (int b = 0; b < 2; b++) {
        LinBuf &B = W.lb[b];
        AL(B.pairM, 27*mx.pair); AL(B.pairCost, mx.pair); AL(B.pairR, 9*mx.pair); AL(B.pairOut, 90*mx.pair);
        AL(B.tgM, 27*mx.tg); AL(B.tgCost, mx.tg);
        AL(B.w_pt, PT_REC*mx.pslot); AL(B.vdb_pt, PT_VDB*(size_t)p->n_pt);
        AL(B.w_tx, TX_REC*mx.tslot); AL(B.V_tx, 6*(size_t)p->n_text); AL(B.b_tx, 3*(size_t)p->n_text); AL(B.dgs_tx, 3*(size_t)p->n_text);
        AL(B.Hd, W.N); AL(B.bp, W.N); AL(B.bp_loc, W.N); AL(B.dgs_p, W.N);
        AL(B.lmpart, 3*((size_t)p->n_pt/64 + (size_t)p->n_text/2 + mx.pair + 8));      // (one partial per k_mid block, at its smallest block size)      // (one partial per k_mid block: at most n_pt / 128 + n_text / 128 + pairs / 128 + 3, and nb_back_max >= n_pt / 64 + n_text / 16)
    }
    AL(W.sig_pt, p->n_pt); AL(W.sig_tx, 3*(size_t)p->n_text); AL(W.sig_p, W.N);
    AL(W.cb, 2*(size_t)W.N + 8); AL(W.cbm, 1);
    return 0;
}
// the layout of the reduced system for the levels on the device (a ring plan is only built for single-level solves)
static SolverLayout upload_layout(const Ctx *c) {
    int ring = 0, ring_k0 = 0; for (int l = 0; l < c->n_levels; l++) if (c->lev_built[l] && c->hplan[l].ring) { ring = 1; ring_k0 = c->hplan[l].ring_k0; }
    return choose_solver_layout(c->n_kf, max_band_rows(c), ring, ring_k0, is_multi(c), c->dbg);
}
// leaves S (dense or band) and the buffers of the solver the layout names: the streaming band solver's factor, the partitioned solver's interiors and separator system
static int alloc_reduced_system(Ctx *c, const tsba_problem *p, const SolverLayout &L) {
    Work &W = c->W; const int bw = L.bw_rows;
    c->lay = L;
    W.dp_poll = L.use_lds && !is_multi(c) && !c->pose_only && (c->dbg.solve_variant == 0 || c->dbg.solve_variant == 5 || c->dbg.solve_variant == 6);        // solver and back-substitution in one launch (k_solve_back)
    if (W.dp_poll) {                           // ... whose workgroups poll the solver's: only where the whole grid is resident at once (else k_solve_t + k_back + k_decide)
        const int ldsb = solve_back_lds_bytes((int)(solve_lds_doubles(W.N)*sizeof(double)), W.N);
        ATTR(k_solve_back<true>, ldsb);
        if (!grid_resident(c, (const void *)k_solve_back<true>, SOLVE_THREADS, (size_t)ldsb, 1 + (c->nb_back_max + 2)/3)) W.dp_poll = 0;
    }
    c->S_up = L.S_up; c->S_count = L.S_count; AL(c->S_alloc, c->S_count);
    if (!L.band) { W.S = c->S_alloc; W.ldS = W.N; W.band = 0; }
    else { W.S = c->S_alloc + (L.LDB - L.S_up); W.ldS = (int)L.LDB - 1; W.band = 1; }
    W.ring = 0; W.ring_g = 0; W.ring_b = 0; W.ring_k0 = -1;
    c->Lcol = nullptr; c->band_stream = L.band_stream; c->sep_cr = L.sep_cr != 0; c->band_parts = L.P;
    if (L.band_stream) AL(c->Lcol, ((size_t)p->n_kf + bw/6 + 1)*bw*6);
    if (L.partitioned) {                       // substructuring: P interiors on P workgroups + a separator system (again a band, 2 bw - 6 wide)
        const int P = L.P, nsep = L.nsep;
        c->nsep_ld = nsep;
        AL(c->Lb, ((size_t)p->n_kf + bw/6 + 1)*bw*6); AL(c->Tbuf, (size_t)P*((size_t)4*bw*bw + 2*bw));
        AL(c->Bpart, (size_t)P*BANDP_NS*((size_t)bw*bw + bw));
        if (L.sep_cr) { AL(c->Ssep, cr_pool_blocks(L.nsepb)*(size_t)bw*bw); AL(c->CRcontrib, (size_t)L.nsepb*cre_contrib_doubles(bw)); AL(c->CRfac, (size_t)L.nsepb*cre_rec_doubles(bw)); AL(c->CRgate, (size_t)(L.nsepb + 2)*TSBA_CRE_KMAX); c->cre_epoch = 0; }
        else AL(c->Ssep, (size_t)nsep*nsep + nsep);
        AL(c->Lcol_sep, (size_t)(nsep/6 + 1)*L.bws*6);
        Work &Ws = c->Wsep; memset(&Ws, 0, sizeof(Ws));
        Ws.N = nsep; Ws.n_kf = 0; Ws.S = c->Ssep; Ws.ldS = nsep; Ws.band = 1; Ws.st = nullptr;       // (st is set at launch: W.st is allocated by alloc_step_buffers)
        AL(Ws.Sy, nsep); AL(Ws.g, nsep); AL(Ws.dp, nsep); AL(Ws.LDbuf, 32*(size_t)(nsep/6 + 1)); AL(Ws.nfree, 1); AL(Ws.fidx, 1);
        W.ring = L.ring; W.ring_g = L.ring_G; W.ring_b = bw/6; W.ring_k0 = L.ring_k0;
    }
    if (L.err) { set_err(c, "ring-shaped map: the partitioned band solver is not available for this plan"); return L.err; }
    AL(W.Sy, W.N + BAND_BW_MAX);                            // (+ the ghost rows of a ring map)
    return 0;
}
// leaves the conjugate-gradient buffers of a map with long-range coupling (tsba_pcg.h) and the packed band rows that several ranks exchange
static int alloc_pcg(Ctx *c, const tsba_problem *p, const SolverLayout &L) {
    Work &W = c->W;
    c->far_B = 0; c->n_far = 0; c->pcg_parts = 0;
    for (int l = 0; l < p->n_levels; l++) if (c->lev_built[l] && c->lev[l].far_B > 0) { c->far_B = c->lev[l].far_B; c->n_far = std::max(c->n_far, c->lev[l].n_far); }
    if (c->far_B > 0) {
        if (!W.band || !c->band_stream) { set_err(c, "map with long-range coupling: the band solvers are not available for this plan"); return TSBA_ERR_STATE; }
        c->pcg_parts = (p->n_kf + 31)/32;
        AL(W.Sfar, 36*(size_t)std::max(c->n_far, 1));
        AL(W.pc_x, W.N); AL(W.pc_r, W.N); AL(W.pc_p[0], W.N); AL(W.pc_p[1], W.N); AL(W.pc_q, W.N); AL(W.pc_g0, W.N);
        AL(W.pc_part, 5*(size_t)c->pcg_parts + 16 + 144); AL(W.pcs, 2); AL(W.pc_stat, 8);       // (pc_part: + partial r.z per interior of the solve phase, tsba_bandsv.h)
    }
    c->S_xchg = nullptr; c->xchg_wp = L.xchg_wp;
    if (L.xchg_wp) AL(c->S_xchg, ((size_t)W.N + L.bw_rows)*L.xchg_wp);
    return 0;
}
// leaves the buffers of an LM step: gradient, pose and landmark steps, the kernels' partial sums, the two copies of the LM state
static int alloc_step_buffers(Ctx *c, const tsba_problem *p, const LevelMax &mx) {
    Work &W = c->W;
    AL(W.g, W.N); AL(W.dp, W.N + 2); AL(W.dl_pt, p->n_pt); AL(W.dl_tx, 3*(size_t)p->n_text);
    AL(W.partial, 2*(size_t)c->nb_back_max);
    AL(W.posepart, 2*((size_t)p->n_kf/21 + 2));
    AL(W.cntpart, 2*(mx.cnt/4 + mx.cnt/256 + 4));
    AL(W.st, 2); c->st_base = W.st; AL(W.dec, 1);
    W.st_next = (W.dp_poll && p->n_kf <= SCHUR_KEEP_KF) ? W.st + 1 : nullptr;        // windows on one GPU: k_schur_t takes the previous trial's decision itself (the two copies of the state swap roles after that launch)
    AL(c->cov_log, 6*TSBA_MAX_LEVELS);
    return 0;
}
// leaves the last staged bytes on their way and the problem marked uploaded.  A resident upload ends synchronised; a one-shot call goes straight on to the solve on
// the same stream: nothing touches the staged bytes before free_problem's synchronisation at the next upload
static int finish_upload(Ctx *c, bool lazy, const UploadTimes &T, PlannerJoiner &joiner) {
    flush_run(c);
    const auto t2 = UpClock::now();
    c->upload_pending = false;
    if (lazy && c->ev_upload && (!c->stage_p || c->copy_stream)) { if (c->stage_p) { hipEventRecord(c->ev_upload, c->stream); c->upload_pending = true; } }
    else if (hipStreamSynchronize(c->stream) != hipSuccess) { set_err(c, "upload sync failed"); return TSBA_ERR_DEVICE; }
    if (T.verbose) fprintf(stderr, "[tsba_upload] free %.2f ms, host total %.2f ms (waiting for the plan threads %.2f ms, image section %.2f ms), final sync %.2f ms\n",
                           ms_between(T.t0, T.t1), ms_between(T.t1, t2), T.plan, T.img, ms_between(t2, UpClock::now()));
    c->uploaded = true;
    joiner.armed = false;                          // (deferred levels: their plan threads are joined by stage_level / free_problem)
    if (!c->stage_p) join_planners(c);
    return TSBA_OK;
}
// lazy: the caller (a one-shot entry point) runs the solve right away and keeps *p alive until it returns -- on small windows only the first
// pass's level is staged here, the others when their pass begins (tsba_solve), so that the coarse passes run on the device while the host
// still builds and stages the plan of level 0 (the largest: ~1 ms of a 20-keyframe window's cold call)
static int upload_impl(void *ctx, const tsba_problem *p, const tsba_options *o, bool lazy) {
    Ctx *c = (Ctx *)ctx; if (!c) return TSBA_ERR_ARG;
    hipSetDevice(c->device);
    int rc = check_problem(c, p, o); if (rc) return rc;
    UploadTimes T; T.verbose = c->dbg.verbose != 0; T.t0 = UpClock::now();
    free_problem(c);
    T.t1 = UpClock::now();
    o = begin_upload(c, p, o);
    PlannerJoiner joiner{c, true};
    const PlanStart plans = start_plans(c, p, o, lazy, T);
    if ((rc = upload_problem_arrays(c, p))) return rc;
    if ((rc = assign_plane_cache(c, p, o))) return rc;
    LevelMax mx;
    if ((rc = stage_levels(c, p, o, plans, &mx, T))) return rc;      // (the first plan behind the problem arrays and the plane cache: a deferring call overlaps their copy)
    if ((rc = alloc_pose_buffers(c, p, mx))) return rc;
    if ((rc = alloc_lin_buffers(c, p, mx))) return rc;
    const SolverLayout L = upload_layout(c);
    if ((rc = alloc_reduced_system(c, p, L))) return rc;
    if ((rc = alloc_pcg(c, p, L))) return rc;
    if ((rc = alloc_step_buffers(c, p, mx))) return rc;
    return finish_upload(c, lazy, T, joiner);
}
int tsba_upload(void *ctx, const tsba_problem *p, const tsba_options *o) { return upload_impl(ctx, p, o, false); }

// leaves D.img: the table of the level's image planes -- staged here, resident already (tsframe_level_ptr), or in the keyframes' slots of the plane cache
static int stage_level_images(Ctx *c, const tsba_problem *p, int l, LevelDev &D) {
    std::vector<const uint8_t *> ptrs(p->n_kf, nullptr);
    const size_t npx = (size_t)p->img_w[l]*p->img_h[l];
    for (int k = 0; k < p->n_kf; k++) {                 // through the pinned staging mirror: one copy for the whole level
        if (!p->img[l][k]) { set_err(c, "null image pointer"); return TSBA_ERR_ARG; }
        if (c->opt.img_on_device) { ptrs[k] = p->img[l][k]; continue; }   // resident pyramid plane (tsframe_level_ptr): used in place
        if (c->use_img_cache) { ptrs[k] = c->ic.dev + (size_t)c->ic_slot[(size_t)k]*c->ic.slot + c->ic.lvl_off[l]; continue; }   // the keyframe's slot of the plane cache (filled by the upload)
        UP(ptrs[k], p->img[l][k], npx);
    }
    const uint8_t *const *dptr = nullptr;
    UP(dptr, (const uint8_t *const *)ptrs.data(), ptrs.size());
    D.img = (const uint8_t *const *)dptr;
    return 0;
}
// One pyramid level onto the device: the plan's lists (its host thread is joined here), the level's reference features, the table of image planes.
static int stage_level(Ctx *c, const tsba_problem *p, int l, double *t_plan, double *t_img) {
    const tsba_options *o = &c->opt; int rc;
    if (c->stage_async && c->copy_stream && c->upload_pending) { hipStreamWaitEvent(c->copy_stream, c->ev_upload, 0); c->upload_pending = false; }
    {   auto tp0 = std::chrono::steady_clock::now();            // in pass order: the coarse levels are ready first and are staged while level 0 is still being built
        if (l < (int)c->planners.size() && c->planners[l].joinable()) c->planners[l].join();
        if (t_plan) *t_plan += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count(); }
    HostPlan &H = c->hplan[l];
    LevelDev &D = c->lev[l]; memset(&D, 0, sizeof(D));
    D.level = l; D.n_sc = H.n_sc(); D.n_pair = H.n_pair(); D.n_tg = H.n_tg(); D.n_pslot = H.n_pslot(); D.n_tslot = H.n_tslot(); D.n_sb = H.n_sb(); D.bw_rows = 6*H.bw_pose;
    for (int k = 0; k < 4; k++) { double v = p->K[k]; for (int q = 0; q < l; q++) v *= 0.5; D.K[k] = v; }
    D.img_w = p->img_w[l]; D.img_h = p->img_h[l];
#define UV(field) do { rc = dev_upload_vec(c, &D.field, H.field); if (rc) return rc; } while (0)
    UV(sc_obs); UV(sc_kf); UV(sc_pt); UV(sc_flag); UV(sc_slot); UV(sc_uv);
    UV(tg_rec); UV(tg_ppos); UV(pt_pose6); UV(pt_pair4); UV(tx_pair8); UV(pair_i); UV(pair_h); UV(pair_hpos); UV(pair_sc_off); UV(pair_tg_off); UV(pair_tg);
    UV(tg_tobs); UV(tg_kf); UV(tg_text); UV(tg_pair); UV(tg_slot);
    UV(pf_g); UV(pf_f); D.n_pf = (int)H.pf_g.size();
    for (int g = 0; g < D.n_tg; g++) D.tg_fmax = std::max(D.tg_fmax, (int)(H.tg_rec[8*(size_t)g + 6] - H.tg_rec[8*(size_t)g + 5]));
    if (!H.kf_order.empty()) UV(kf_order); else D.kf_order = nullptr;
    D.far_B = H.far_B; D.n_far = H.n_far();
    D.sb_far = nullptr;
    D.n_wb = (int)H.wb_kf.size(); D.wb_kf = nullptr; D.wb_idx = nullptr;
    if (H.far_B > 0 && D.n_wb > 0) { UV(wb_kf); UV(wb_idx); }
    D.far_rec = nullptr; D.n_far_ent = H.far_B > 0 ? (int)H.far_ent.size() : 0;
    if (H.far_B > 0) { rc = dev_alloc(c, &D.far_rec, std::max<size_t>(1, H.far_ent.size())); if (rc) return rc; }
    if (H.far_B > 0) { UV(far_a); UV(far_b); UV(far_off); UV(far_ent); UV(fb_id); UV(fb_pab); UV(fb_pba); UV(fb_pt_off); UV(fb_pt_s1); UV(fb_pt_s2); UV(fb_pt_lm);
        UV(fb_tx_off); UV(fb_tx_s1); UV(fb_tx_s2); UV(fb_tx_lm); }
    UV(pls_off); UV(pslot_pose); UV(pslot_pair); UV(pslot_lm); UV(tls_off); UV(tslot_pose); UV(tslot_pair); UV(tslot_lm);
    UV(sb_a); UV(sb_b); UV(sb_pab); UV(sb_pba); UV(sb_rng); UV(sb_tx_off); UV(sb_tx_s1); UV(sb_tx_s2); UV(sb_tx_lm);
    int *dp_off = nullptr, *dp_s1 = nullptr, *dp_s2 = nullptr, *dp_lm = nullptr; const int32_t *dp_cl = nullptr;
    if (H.dev_pt_pairs >= 0) {                                     // large maps: the point slot pairs by block are built on the device (tsba_devplan.h)
        rc = dev_alloc(c, &dp_off, (size_t)D.n_sb + 2); if (rc) return rc;
        const size_t tot = (size_t)std::max<int64_t>(H.dev_pt_pairs, 1);
        rc = dev_alloc(c, &dp_s1, tot); if (rc) return rc; rc = dev_alloc(c, &dp_s2, tot); if (rc) return rc; rc = dev_alloc(c, &dp_lm, tot); if (rc) return rc;
        if (!H.cl_pt_dev.empty()) { rc = dev_upload_vec(c, &dp_cl, H.cl_pt_dev); if (rc) return rc; }
        D.sb_pt_off = dp_off; D.sb_pt_s1 = dp_s1; D.sb_pt_s2 = dp_s2; D.sb_pt_lm = dp_lm;
    } else { UV(sb_pt_off); UV(sb_pt_s1); UV(sb_pt_s2); UV(sb_pt_lm); }
    UV(pose_t_off); UV(pose_t); UV(pose_h_off); UV(pose_h); UV(pose_ps_off); UV(pose_ps); UV(pose_ps_lm); UV(pose_ts_off); UV(pose_ts); UV(pose_ts_lm);
#undef UV
    if (p->n_text > 0 && p->tfeat_off[l]) {
        D.n_tfeat = p->n_tfeat[l];
        UP(D.tfeat_off, p->tfeat_off[l], (size_t)p->n_text + 1); UP(D.tfeat_raw, p->tfeat_raw[l], p->n_tfeat[l]);
        UP(D.tfeat_uv, p->tfeat_uv[l], 2*(size_t)p->n_tfeat[l]); UP(D.tfeat_ref, p->tfeat_ref[l], 8*(size_t)p->n_tfeat[l]);
    } else { std::vector<int32_t> z((size_t)p->n_text + 1, 0); UP(D.tfeat_off, z.data(), z.size()); }
    auto ti0 = std::chrono::steady_clock::now();
    if (o->use_text && p->n_tobs > 0 && p->img[l]) { rc = stage_level_images(c, p, l, D); if (rc) return rc; }
    if (t_img) *t_img += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ti0).count();
    if (c->stage_async || H.dev_pt_pairs >= 0) flush_run(c);        // (a level staged with the upload: its bytes leave with the upload's last copy -- one copy for all levels of a single-frame call)
    if (H.dev_pt_pairs >= 0 && D.n_sb > 0) {                       // (after the copies it reads, on the stream they went over)
        hipStream_t sq = c->stage_async && c->copy_stream ? c->copy_stream : c->stream;
        hipMemsetAsync(dp_off, 0, sizeof(int)*((size_t)D.n_sb + 2), sq);
        LAUNCHK(k_sb_pairs<0>, dim3(D.n_sb), dim3(64), 0, sq, D.n_sb, D.sb_a, D.sb_b, D.pose_ps_off, D.pose_ps, D.pose_ps_lm, D.pls_off, D.pslot_pose, (const int *)dp_cl, dp_off, dp_s1, dp_s2, dp_lm);
        LAUNCHK(k_sb_scan, dim3(1), dim3(1024), 0, sq, D.n_sb, dp_off);
        LAUNCHK(k_sb_pairs<1>, dim3(D.n_sb), dim3(64), 0, sq, D.n_sb, D.sb_a, D.sb_b, D.pose_ps_off, D.pose_ps, D.pose_ps_lm, D.pls_off, D.pslot_pose, (const int *)dp_cl, dp_off, dp_s1, dp_s2, dp_lm);
    }
    if (c->stage_async && c->copy_stream && c->ev_stage[l]) { hipEventRecord(c->ev_stage[l], c->copy_stream); c->lev_wait[l] = 1; }      // the level's pass waits for this copy
    c->lev_built[l] = 1;
    return TSBA_OK;
}
#undef UP
#undef UPZ
#undef AL
// during a solve: levels of later passes whose plans are complete go to the device now, over the copy stream, next to the running pass
static int stage_ahead(Ctx *c, int ps) {
    if (!c->stage_p) return TSBA_OK;
    for (int q = ps + 1; q < c->opt.n_passes; q++) { const int l = c->opt.levels[q];
        if (c->lev_built[l] || !c->lev_planned[l]) continue;
        if (!c->plan_done[l].load(std::memory_order_acquire)) break;           // in pass order
        c->stage_async = true; const int rc = stage_level(c, c->stage_p, l, nullptr, nullptr); c->stage_async = false;
        if (rc) return rc; }
    return TSBA_OK;
}

static int reset_state(Ctx *c) {                 // one launch instead of ten small copies (each ~2.5 us on the stream)
    Work &W = c->W;
    ResetSrc A = { (const double *)c->pose0, (const double *)c->rho0, (const double *)c->theta0,
                   (const uint8_t *)c->sgood0, (const uint8_t *)c->tobs_good0, (const uint8_t *)c->tfgood0,
                   (long long)7*c->n_kf, (long long)c->n_pt, (long long)3*c->n_text, (long long)c->n_sgood, (long long)c->n_tobs, (long long)c->n_tfgood };
    long long mx = std::max(std::max(A.n_pose, A.n_rho), std::max(std::max(A.n_theta, A.n_sg), std::max(A.n_tg, A.n_tf)));
    const int nb = (int)std::min<long long>(1024, std::max<long long>(1, (mx + 255)/256));
    LAUNCHK(k_reset_state, dim3(nb), dim3(256), 0, c->stream, W, A);
    return 0;
}

static bool is_multi(const Ctx *c) { return c->world > 1 || c->force_multi; }

// In-process communicator (tsba_comm_init_local): `world` contexts of one process, one host thread each.  A collective is
// stream-sync -> device-to-host -> barrier -> rank 0 reduces in rank order (deterministic) -> barrier -> host-to-device.
// It exists so that the N > 1 code path -- sharded upload, split kernel sequence, every exchange -- runs under the test-suite on a
// one-GPU box; production multi-GPU runs use RCCL (tsba_comm_init).
struct LocalGroup {
    int world = 1; bool broken = false;
    std::vector<Ctx *> members;                    // contexts that joined (tsba_comm_init_local): their lgroup is cleared when the group goes away
    std::mutex m; std::condition_variable cv; int arrived = 0; unsigned long long gen = 0;
    std::vector<std::vector<char>> stage; std::vector<char> result;
    // The ranks of a group usually share ONE device.  A rank holds this token while it has kernels in flight (from the moment it leaves a
    // collective until its stream has drained at the next one), so that the ranks' launches do not overlap on the device: kernel
    // durations under a profiler are then those of a rank that has the GPU to itself, as in a real multi-GPU run.
    std::mutex gpu_token;
    void fail() { std::lock_guard<std::mutex> lk(m); broken = true; cv.notify_all(); }     // a member gives up: the others must not wait for it
    bool barrier() {                               // false: a member never arrived (it failed before the collective) -- do not hang
        std::unique_lock<std::mutex> lk(m);
        if (broken) return false;
        const unsigned long long g = gen;
        if (++arrived == world) { arrived = 0; gen++; cv.notify_all(); return true; }
        if (!cv.wait_for(lk, std::chrono::seconds(120), [&] { return gen != g || broken; })) { broken = true; cv.notify_all(); return false; }
        return !broken;
    }
};
static void lgroup_forget(Ctx *c) {              // the context leaves its in-process group (destroyed, or joined to an RCCL communicator)
    if (!c->lgroup) return;
    { std::lock_guard<std::mutex> lk(c->lgroup->m); for (Ctx *&m : c->lgroup->members) if (m == c) m = nullptr; }
    c->lgroup = nullptr;
}
static void local_allreduce(Ctx *c, void *buf, size_t count, ncclDataType_t dt, ncclRedOp_t op) {
    LocalGroup *G = c->lgroup;
    const size_t bytes = count*(dt == ncclDouble ? sizeof(double) : sizeof(int));
    auto fail = [&](const char *what) { c->err = std::string("ncclAllReduce (local group): ") + what; G->fail(); };
    if (hipStreamSynchronize(c->stream) != hipSuccess) { fail("stream"); return; }
    std::vector<char> &mine = G->stage[c->rank];
    mine.resize(bytes);
    if (hipMemcpy(mine.data(), buf, bytes, hipMemcpyDeviceToHost) != hipSuccess) { fail("device-to-host"); return; }
    if (c->has_token) { c->has_token = false; G->gpu_token.unlock(); }          // this rank's kernels have drained: the next rank may run
    struct Retake { Ctx *c; LocalGroup *G; ~Retake() { if (c->in_solve && !c->has_token) { G->gpu_token.lock(); c->has_token = true; } } } retake{c, G};
    if (!G->barrier()) { fail("a rank did not arrive"); return; }
    if (c->rank == 0) {
        G->result = G->stage[0];
        for (int r = 1; r < G->world; r++) {
            if (G->stage[r].size() != bytes) { G->fail(); break; }              // ranks disagree on the count: a layout bug, never sum garbage
            if (dt == ncclDouble) { double *a = (double *)G->result.data(); const double *b = (const double *)G->stage[r].data();
                if (op == ncclMax) for (size_t k = 0; k < count; k++) a[k] = a[k] > b[k] ? a[k] : b[k]; else for (size_t k = 0; k < count; k++) a[k] += b[k]; }
            else { int *a = (int *)G->result.data(); const int *b = (const int *)G->stage[r].data(); for (size_t k = 0; k < count; k++) a[k] += b[k]; }
        }
    }
    if (!G->barrier()) { fail("ranks disagree on the element count, or a rank did not arrive"); return; }
    if (hipMemcpy(buf, G->result.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) fail("host-to-device");
}
static void allreduce(Ctx *c, void *buf, size_t count, ncclDataType_t dt, ncclRedOp_t op) {
    c->x_acc += count*(dt == ncclDouble ? sizeof(double) : sizeof(int));
    if (c->lgroup) { local_allreduce(c, buf, count, dt, op); return; }
    if (!c->comm) return;                          // force_multi without a communicator: exercises the split kernels only
    ncclResult_t r = c->p_allreduce(buf, buf, count, dt, op, c->comm, c->stream);
    if (r != ncclSuccess) c->err = std::string("ncclAllReduce: ") + c->p_errstr(r);
}
static void launch_pass_init(Ctx *c, const LevelDev &D, int pass) {
    const size_t x0 = c->x_acc;
    struct XP { Ctx *c; size_t x0; ~XP() { c->x_pass = c->x_acc - x0; } } xp{c, x0};
    c->cur_bw_rows = D.bw_rows; c->S_stale = true;             // (a new pass: other free poses, other entries of S)
    c->W.hprog = c->hprog; c->W.pass_seq = ++c->pass_seq; c->W.trace_pass = pass;
    Work &W = c->W; const tsba_options &o = c->opt;
    LAUNCHK(k_pass_reset, dim3(64), dim3(256), 0, c->stream, W, o.initial_radius, o.its[pass]);
    int n = D.n_sc + D.n_tg;
    const int npb = (D.n_sc + 255)/256 + (D.n_tg + 3)/4;                    // k_participation workgroups: scene candidates | text groups
    const int ncp = (n > 0 && !is_multi(c)) ? npb : 0;                      // count partials (single GPU)
    if (n > 0) LAUNCHK(k_participation, dim3(npb), dim3(256), 0, c->stream, W, D, ncp ? 1 : 0);
    if (is_multi(c)) {                             // participation and block counts are global properties
        allreduce(c, W.kf_in, c->n_kf, ncclInt32, ncclSum);
        allreduce(c, &W.st->ns_active, 2, ncclInt32, ncclSum);
        LAUNCHK(k_kfin_multi, dim3((c->n_kf + 255)/256), dim3(256), 0, c->stream, W);
    }
    if (c->n_kf <= 64) LAUNCHK(k_gauge_wave, dim3(1), dim3(64), 0, c->stream, W, (const uint8_t *)c->kf_initial, o.state, ncp);
    else if (c->n_kf > 256) LAUNCHK(k_gauge_par, dim3(1), dim3(1024), 0, c->stream, W, (const uint8_t *)c->kf_initial, o.state, ncp, D.kf_order);
    else LAUNCHK(k_gauge, dim3(1), dim3(64), 0, c->stream, W, (const uint8_t *)c->kf_initial, o.state, ncp, D.kf_order);
    if (D.far_B > 0 && D.far_rec) { const int ne = D.n_far_ent;      // the blocks outside the band by keyframe, with the other keyframe's row (the gauge is fixed now)
        if (ne > 0) LAUNCHK(k_far_rows, dim3((ne + 255)/256), dim3(256), 0, c->stream, W, D, ne); }
    if (D.n_tg > 0) LAUNCHK(k_musigma, dim3(D.n_tg), dim3(MS_THREADS), 0, c->stream, W, D);
}
// k_mid's blocks: 256 landmarks / pairs each.  tsba_debug_options.trial_launches = 1 / 2 (the k_lin_mid experiment and its comparison partner): 128 (MID_TW: what a
// workgroup of the linearisation can take over)
// Windows (round 6): ONE wave per block -- what bounds a block is the number of cache lines its gathers pull through its compute unit's vector cache (256 points x 5 slots
// x (a 64-byte record + a 72-byte rotation) took ~10 k cycles on each of 20 compute units); 64-thread blocks put the same gathers on four times as many
static int mid_threads(const Ctx *c) { return c->n_kf <= SCHUR_KEEP_KF ? ((c->dbg.trial_launches == 1 || c->dbg.trial_launches == 2) ? MID_TW : 64) : 256; }
// (round 6: a plane has MID_PL = 8 lanes, one slot record each, a pair MID_PR = 4 lanes that share its text groups: the three kinds of block each end after
// two dependent round trips instead of up to eight)
static void mid_blocks(const Ctx *c, const LevelDev &D, int &nb_pt, int &nb_tx, int &nb_pr) { const int t = mid_threads(c);
    const int pr = MID_PR_MIN;
    nb_pt = (c->n_pt + t - 1)/t;
    if (t == 64) { nb_tx = (c->n_text + 1)/2; nb_pr = D.n_pair; }      // one-wave blocks: a plane on 32 lanes, a pair on the whole wave (a lane per value / output)
    else { nb_tx = (c->n_text + t/MID_PL - 1)/(t/MID_PL); nb_pr = (D.n_pair + t/pr - 1)/(t/pr); } }
static int pose_parts(const Ctx *c) { return c->n_kf > 126 ? (c->n_kf + 20)/21 : 0; }    // k_pose_sums workgroups (0: the pose sums stay in k_postlin / k_decide)
// pairs with a dozen scene blocks (large maps): four pairs per wave
static bool lin_small_pairs(const Ctx *c, const LevelDev &D) { return !c->dbg.no_small_pairs && D.n_pair > 0 && (long long)D.n_sc <= 24LL*D.n_pair; }
static bool fused_decisions(const Ctx *c, const LevelDev &D);
// tsba_debug_options.trial_launches = 4 / 5: production's launches with a comparison partner of k_linearize's text lanes (lin_body<.., VAR>) -- 4: every tap projected
// twice (LIN_REDO: the carried projection's partner); 5: a wave without a feature evaluates the clamped last feature under weight 0 (LIN_ALLW: the idle-wave skip's partner)
static int lin_variant(const Ctx *c) { return c->dbg.trial_launches == 4 ? LIN_REDO : c->dbg.trial_launches == 5 ? LIN_ALLW : LIN_PROD; }
// production's launch sequence (148 launches per C4 solve, the decision block in k_mid's launch): production itself and the partners that differ inside k_linearize only
static bool production_launches(const Ctx *c) { return c->dbg.trial_launches == 0 || lin_variant(c) != LIN_PROD; }
// windows on one GPU with one-wave k_mid blocks: a speculative k_mid launch carries the decision block (decision_block, tsba_kernels_lin.h) and the k_schur_t<4>
// behind it reads the record it leaves (SchurDec.on = 3).  tsba_debug_options.trial_launches = 1 / 2 (128-thread blocks, k_lin_mid) keep the decision inside k_schur_t (on = 1)
static bool decision_in_mid(const Ctx *c, const LevelDev &D) { return fused_decisions(c, D) && mid_threads(c) == 64; }
// one-wave workgroups (LIN_T1) where a wave takes a whole pair and the level's largest text group fits one wave's feature places (production only: the partners keep both waves)
static bool lin_one_wave(const Ctx *c, const LevelDev &D) { return !lin_small_pairs(c, D) && lin_variant(c) == LIN_PROD && D.n_tg > 0 && D.tg_fmax <= LIN_T1/(8/LIN_TPL); }
// k_linearize of a level: the instantiation and the grid by the level's shape (pairs with a dozen scene blocks: four per wave -- without text groups the scene path's
// registers only; small text groups: one-wave workgroups) and by lin_variant
static void launch_k_linearize(Ctx *c, const LevelDev &D, int spec) {
    const int ppw = lin_small_pairs(c, D) ? 4 : 1, var = lin_variant(c), nt = lin_one_wave(c, D) ? LIN_T1 : LIN_T, nwv = nt/64;
    const dim3 g((((D.n_pair + ppw*nwv - 1)/(ppw*nwv) + D.n_tg + 7)/8)*8);
#define LIN_LAUNCH(PPW, ...) LAUNCHK((k_linearize<MODE_FULL, PPW, __VA_ARGS__>), g, dim3(nt), 0, c->stream, c->W, D, spec)
    if (nt == LIN_T1) LIN_LAUNCH(1, true, LIN_PROD, LIN_T1);
    else if (ppw == 4 && D.n_tg == 0) LIN_LAUNCH(4, false);
    else if (ppw == 4) { if (var == LIN_REDO) LIN_LAUNCH(4, true, LIN_REDO); else if (var == LIN_ALLW) LIN_LAUNCH(4, true, LIN_ALLW); else LIN_LAUNCH(4, true, LIN_PROD); }
    else { if (var == LIN_REDO) LIN_LAUNCH(1, true, LIN_REDO); else if (var == LIN_ALLW) LIN_LAUNCH(1, true, LIN_ALLW); else LIN_LAUNCH(1, true, LIN_PROD); }
#undef LIN_LAUNCH
}
static void launch_linearize(Ctx *c, const LevelDev &D, int spec, bool skip_postlin = false) {      // skip_postlin: windows -- the first k_schur_t of the pass does k_postlin's work (SchurDec.on = 2)
    struct XL { Ctx *c; size_t x0; ~XL() { c->x_lin = c->x_acc - x0; } } xl{c, c->x_acc};
    Work &W = c->W;
    int nb_pt, nb_tx, nb_pr; mid_blocks(c, D, nb_pt, nb_tx, nb_pr); const int nb_kf = (c->n_kf + 255)/256;
    // EXPERIMENT, off by default (trial_launches = 2): k_mid inside the speculative linearisation's launch (k_lin_mid: its last workgroups to finish take the k_mid
    // blocks).  Measured in round 5: 40.7 us per launch against 13.4 + 10.6 us for the two launches -- 736 workgroups telling each other that they are done costs
    // more than the kernel boundary it replaces (tools/ticket_bench.hip, docs/ledger_r05.md 14.2)
    const unsigned lm_grid = (unsigned)((((D.n_pair + LIN_NWV - 1)/LIN_NWV + D.n_tg + 7)/8)*8);
    if (spec && W.st_next && c->lin_ticket && c->dbg.trial_launches == 2 && !is_multi(c) && mid_threads(c) == MID_TW && D.n_pair + D.n_tg > 0 && !lin_small_pairs(c, D)
        && grid_resident(c, (const void *)k_lin_mid, LIN_T, 0, (int)lm_grid)) {      // (its retained workgroups wait for every arrival: only where the whole grid is resident, as every launch that waits)
        const unsigned grid = lm_grid;
        LAUNCHK(k_lin_mid, dim3(grid), dim3(LIN_T), 0, c->stream, W, D, nb_pt, nb_tx, nb_pt + nb_tx + nb_pr, c->lin_ticket, c->lin_base);
        c->lin_base += grid;
        return;
    }
    if (D.n_pair + D.n_tg > 0) launch_k_linearize(c, D, spec);
    const MidDec md0{0, 0, 0, tsba_options{}};
    if (mid_threads(c) == MID_TW) LAUNCHK((k_mid<MID_TW, 6, MID_PR_MIN>), dim3(nb_pt + nb_tx + nb_pr), dim3(MID_TW), 0, c->stream, W, D, nb_pt, nb_tx, spec, md0);
    else if (mid_threads(c) == 64) {                  // (a speculative launch: + the decision block, which takes the trial's light decision for the next k_schur_t<4>)
        const int dec_on = spec && decision_in_mid(c, D) ? 1 : 0;
        LAUNCHK((k_mid<64, 6, MID_PR_MIN>), dim3(nb_pt + nb_tx + nb_pr + dec_on), dim3(64), 0, c->stream, W, D, nb_pt, nb_tx, spec,
                dec_on ? MidDec{1, nb_pr, back_blocks_pt(c->n_pt) + back_blocks_tx(c->n_text) + nb_kf, c->opt} : md0);
    } else LAUNCHK((k_mid<256, 4, MID_PR_MIN>), dim3(nb_pt + nb_tx + nb_pr), dim3(256), 0, c->stream, W, D, nb_pt, nb_tx, spec, md0);
    const int multi = is_multi(c);
    const int npp = pose_parts(c);
    if (multi) {
        // local sums -> exchange buffer -> all-reduce; the consumer (k_postlin / k_decide) installs them into the right LinBuf
        if (npp) LAUNCHK(k_pose_sums_raw, dim3(npp), dim3(256), 0, c->stream, W, D, spec);
        LAUNCHK(k_sums_multi, dim3(1), dim3(256), 0, c->stream, W, D, spec, nb_pt + nb_tx + nb_pr, back_blocks_pt(c->n_pt) + back_blocks_tx(c->n_text) + nb_kf, back_blocks_pt(c->n_pt) + back_blocks_tx(c->n_text), npp);      // (k_back's blocks: its partial sums)
        allreduce(c, W.cb, 2*(size_t)W.N + 8, ncclDouble, ncclSum);
        allreduce(c, W.cbm, 1, ncclDouble, ncclMax);
        if (npp) LAUNCHK(k_pose_scale_multi, dim3(npp), dim3(256), 0, c->stream, W, spec);
    } else if (npp) LAUNCHK(k_pose_sums, dim3(npp), dim3(256), 0, c->stream, W, D, spec);
    if (!spec && !skip_postlin) LAUNCHK(k_postlin, dim3(1), dim3(256), 0, c->stream, W, D, c->opt.gradient_tolerance, nb_pt + nb_tx + nb_pr, multi, npp);
}
static int solve_lds_bytes(Ctx *c, int *use_lds) {
    *use_lds = lds_solver_fits(c->W.N);
    return *use_lds ? (int)(solve_lds_doubles(c->W.N)*sizeof(double)) : 0;
}
static int chol_subst_lds_bytes() { return (CH_NB*(CH_NB + 1) + 2*CH_NB + 8*CH_NB)*(int)sizeof(double); }      // k_chol_fwd, k_chol_backsub
static void launch_schur(Ctx *c, const LevelDev &D, int multi, SchurDec dec = SchurDec{0, 0, 0, tsba_options{}}) {
    if (c->n_kf > 126 && !c->dbg.no_schur_quad) {               // large maps: four S blocks per wave, then one wave per pose for the reduced gradient
        const int nq = D.n_sb > 0 ? (((D.n_sb + 3)/4 + 7)/8)*8 : 0, ng = ((c->n_kf + 7)/8)*8;           // (multiples of 8 workgroups: the kernel's XCD-aware mappings)
        if (D.n_tg > 0) LAUNCHK(k_schur_quad<true>, dim3(nq + ng), dim3(64), 0, c->stream, c->W, D, multi, nq, ng);
        else LAUNCHK(k_schur_quad<false>, dim3(nq + ng), dim3(64), 0, c->stream, c->W, D, multi, nq, ng);
    } else if (c->n_kf > 126) LAUNCHK(k_schur_t<1>, dim3(D.n_sb + c->n_kf), dim3(64), 0, c->stream, c->W, D, multi, 0, SchurDec{0, 0, 0, tsba_options{}});
    else LAUNCHK(k_schur_t<4>, dim3(D.n_sb + c->n_kf + (dec.on == 3 ? 1 : 0)), dim3(256), 0, c->stream, c->W, D, multi, 0, dec);      // (on = 3: + the workgroup of the full decision)
    if (D.far_B > 0 && D.n_far > 0) {            // the blocks of E (what couples different clusters of a landmark): the same kernels on the fb_* lists, stored to W.Sfar
        LevelDev E = D;
        E.n_sb = D.n_far; E.sb_a = D.far_a; E.sb_b = D.far_b; E.sb_pab = D.fb_pab; E.sb_pba = D.fb_pba; E.sb_far = D.fb_id;
        E.sb_pt_off = D.fb_pt_off; E.sb_pt_s1 = D.fb_pt_s1; E.sb_pt_s2 = D.fb_pt_s2; E.sb_pt_lm = D.fb_pt_lm;
        E.sb_tx_off = D.fb_tx_off; E.sb_tx_s1 = D.fb_tx_s1; E.sb_tx_s2 = D.fb_tx_s2; E.sb_tx_lm = D.fb_tx_lm;
        if (c->n_kf > 126 && !c->dbg.no_schur_quad) { const int nq = (((E.n_sb + 3)/4 + 7)/8)*8;
            if (D.n_tg > 0) LAUNCHK(k_schur_quad<true>, dim3(nq), dim3(64), 0, c->stream, c->W, E, multi, nq, 0);
            else LAUNCHK(k_schur_quad<false>, dim3(nq), dim3(64), 0, c->stream, c->W, E, multi, nq, 0); }
        else if (c->n_kf > 126) LAUNCHK(k_schur_t<1>, dim3(E.n_sb), dim3(64), 0, c->stream, c->W, E, multi, 0, SchurDec{0, 0, 0, tsba_options{}});
        else LAUNCHK(k_schur_t<4>, dim3(E.n_sb), dim3(256), 0, c->stream, c->W, E, multi, 0, SchurDec{0, 0, 0, tsba_options{}});
    }
}
// kernels with more than 64 KB of dynamic LDS need the attribute once per process
static int set_solver_attrs(Ctx *c) {
    int use_lds; int lds = solve_lds_bytes(c, &use_lds);
    if (use_lds) { ATTR(k_solve_t<false>, lds);
        ATTR((k_solve_t<false, false>), lds);
        ATTR(k_solve_back<true>, solve_back_lds_bytes(lds, c->W.N));
        ATTR(k_solve_back<false>, solve_back_lds_bytes(lds, c->W.N));
        ATTR((k_solve_back<true, true>), solve_back_lds_bytes(lds, c->W.N));
        ATTR(k_solve_la, (int)std::min<size_t>(solve_la_lds_doubles(c->W.N)*sizeof(double), 160*1024 - 64)); }
    else {
        ATTR(k_band_solve, 156*1024);
        ATTR(k_bandp_factor, 156*1024);
        ATTR(k_cr_pivot, 156*1024);
        ATTR(k_cr_update, 156*1024);
        ATTR(k_cr_back, 156*1024);
        ATTR(k_cre_elim, 156*1024);
        ATTR(k_bandp_sepf, 156*1024);
        ATTR(k_cre_back, 156*1024);
        ATTR(k_ms_cre_back, 159*1024);
        ATTR(k_ms_cre_fwd, 100*1024);
        ATTR(k_ms_cre_root, 100*1024);
        ATTR(k_sv_linv, 156*1024);
#define MX_ATTR(SS) ATTR(k_mx_cre_fwd<SS>, 156*1024); ATTR(k_mx_cre_root<SS>, 156*1024); ATTR(k_mx_cre_back<SS>, 156*1024);
        MX_ATTR(36) MX_ATTR(42) MX_ATTR(48) MX_ATTR(54) MX_ATTR(60) MX_ATTR(66)
#undef MX_ATTR
        ATTR(k_sv_fwd_int<1>, 156*1024); ATTR(k_sv_fwd_int<2>, 156*1024);
        ATTR(k_sv_back_int<1>, 156*1024); ATTR(k_sv_back_int<2>, 156*1024);
        ATTR(k_sv_tree_back<1>, 150*1024); ATTR(k_sv_tree_back<2>, 150*1024);
        ATTR(k_bandp_backsub<1>, 156*1024); ATTR(k_bandp_backsub<2>, 156*1024);
        ATTR(k_band_backsub<1>, 156*1024); ATTR(k_band_backsub<2>, 156*1024); ATTR(k_band_backsub<3>, 156*1024);
        ATTR(k_solve_t<true>, (int)(solve_diag_lds_doubles()*sizeof(double)));
        ATTR(k_chol_panel, (CH_NB + 64)*(CH_NB + 1)*(int)sizeof(double));
        ATTR(k_chol_update, 2*64*(CH_NB + 1)*(int)sizeof(double));
        ATTR(k_chol_backsub, chol_subst_lds_bytes()); ATTR(k_chol_fwd, chol_subst_lds_bytes());
    }
    return 0;
}
#include "tsba_solve_launch.h"      // what a trial's reduced-system solve enqueues: launch_solve, the solve phases, launch_solve_full

// a trial's decision is taken by the NEXT trial's k_schur_t (the last trial's by k_decide after the loop, or -- window_pass, decision_in_mid -- by a workgroup of k_pass_end): windows on one GPU without blocks outside the band
static bool fused_decisions(const Ctx *c, const LevelDev &D) { return c->W.st_next != nullptr && D.far_B <= 0; }
// ... and there a pass begins and ends with one launch each (k_pass_begin, k_pass_end).  window_fast_ctx: what the context alone says, for a level that is not on the device yet (only inside a one-shot call: W.st_next is this problem's)
static bool window_fast_ctx(const Ctx *c, bool per_step) { return c->W.st_next != nullptr && c->n_kf <= 64 && !is_multi(c) && !c->pose_only && !per_step; }
static bool window_fast(const Ctx *c, const LevelDev &D, bool per_step) { return window_fast_ctx(c, per_step) && D.far_B <= 0 && D.n_sc + D.n_tg > 0; }
static void launch_decide(Ctx *c, const LevelDev &D) {
    Work &W = c->W;
    int nb_pt, nb_tx, nb_pr; mid_blocks(c, D, nb_pt, nb_tx, nb_pr); const int nb_kf = (c->n_kf + 255)/256;
    const int nb_all = back_blocks_pt(c->n_pt) + back_blocks_tx(c->n_text) + nb_kf;
    LAUNCHK(k_decide, dim3(1), dim3(256), 0, c->stream, W, D, nb_all, nb_pt + nb_tx + nb_pr, c->opt, (int)is_multi(c), pose_parts(c));
}
// one LM iteration: reduced system -> pose step -> back-substitution / candidate -> speculative linearisation at the
// candidate -> decision (on acceptance the speculative LinBuf simply becomes the current one)
static void launch_step(Ctx *c, const LevelDev &D, bool decide_prev = false, bool first_fused = false) {
    struct XT { Ctx *c; size_t x0; ~XT() { c->x_trial = c->x_acc - x0; } } xt{c, c->x_acc};
    Work &W = c->W;
    int nb_pt, nb_tx, nb_pr; mid_blocks(c, D, nb_pt, nb_tx, nb_pr); const int nb_kf = (c->n_kf + 255)/256;
    // block-sparse S: what no block of the plan covers must read as zero.  The streaming / partitioned band solvers leave S intact and a pass
    // writes the same entries in every trial (the free poses are fixed at its start), so the band is cleared once per pass; the in-place
    // Cholesky of the wide-band path needs it before every assembly -- and so does a sharded run (a rank assembles only its own blocks; the
    // other entries hold the sums the last exchange unpacked)
    if ((int64_t)D.n_sb < (int64_t)c->n_kf*(c->n_kf + 1)/2 && (!c->band_stream || c->S_stale || is_multi(c))) {
        hipMemsetAsync(c->S_alloc, 0, sizeof(double)*c->S_count, c->stream); c->S_stale = false;
        if (D.far_B > 0) hipMemsetAsync(W.Sfar, 0, sizeof(double)*36*(size_t)std::max(D.n_far, 1), c->stream); }
    const int bb_pt = back_blocks_pt(c->n_pt), bb_tx = back_blocks_tx(c->n_text), nb_all = bb_pt + bb_tx + nb_kf;      // k_back's blocks
    const bool fused_decide = fused_decisions(c, D);
    if (fused_decide && (decide_prev || first_fused)) {     // (first_fused: the pass's first trial -- workgroup 0 of the assembly does k_postlin's work on the first linearisation, nobody decides anything)
        launch_schur(c, D, 0, SchurDec{decide_prev ? (decision_in_mid(c, D) ? 3 : 1) : 2, nb_all, nb_pt + nb_tx + nb_pr, c->opt});
        std::swap(W.st, W.st_next);                 // from here on the launches see the state that launch wrote
    } else launch_schur(c, D, (int)is_multi(c));
    if (is_multi(c)) {                             // one exchange per LM trial: the reduced normal equations
        if (c->S_xchg) {                           // band storage: only the band's entries travel
            const size_t nx = ((size_t)W.N + (W.ring ? c->xchg_wp - 6 : 0))*c->xchg_wp;
            const int nbp = (int)std::min<size_t>(2048, (nx + 255)/256);
            LAUNCHK(k_band_pack, dim3(nbp), dim3(256), 0, c->stream, W, c->S_xchg, c->xchg_wp, 0);
            allreduce(c, c->S_xchg, nx, ncclDouble, ncclSum);
            LAUNCHK(k_band_pack, dim3(nbp), dim3(256), 0, c->stream, W, c->S_xchg, c->xchg_wp, 1);
        } else allreduce(c, c->S_alloc, c->S_count, ncclDouble, ncclSum);
        if (D.far_B > 0 && D.n_far > 0) allreduce(c, W.Sfar, 36*(size_t)D.n_far, ncclDouble, ncclSum);      // the blocks outside the band
        allreduce(c, W.g, W.N, ncclDouble, ncclSum);
        LAUNCHK(k_damp_multi, dim3((c->n_kf + 255)/256), dim3(256), 0, c->stream, W);
    }
    if (W.dp_poll && D.far_B <= 0) {               // small window: solver (workgroup 0) and back-substitution (three blocks per workgroup, polling the step) in one launch
        int use_lds; const int lds = solve_lds_bytes(c, &use_lds);
        const int ldsb = solve_back_lds_bytes(lds, W.N);
        if (c->dbg.solve_variant == 6) LAUNCHK((k_solve_back<true, true>), dim3(1 + (nb_all + 2)/3), dim3(SOLVE_THREADS), ldsb, c->stream, W, D, bb_pt, bb_tx, nb_all);      // (A/B: the solver workgroup's load and publication as they were before the load by rows)
        else if (c->dbg.solve_variant == 5) LAUNCHK(k_solve_back<false>, dim3(1 + (nb_all + 2)/3), dim3(SOLVE_THREADS), ldsb, c->stream, W, D, bb_pt, bb_tx, nb_all);      // (A/B: the diagonal blocks through the LDS scratch)
        else LAUNCHK(k_solve_back<true>, dim3(1 + (nb_all + 2)/3), dim3(SOLVE_THREADS), ldsb, c->stream, W, D, bb_pt, bb_tx, nb_all);
    } else {
        launch_solve_full(c, D);
        LAUNCHK(k_back, dim3(nb_all), dim3(256), 0, c->stream, W, D, bb_pt, bb_tx);
    }
    launch_linearize(c, D, 1);
    if (!fused_decide) launch_decide(c, D);
}

// ---- the solve: one driver per kind of pass (pose_pass, window_pass, generic_pass), each from its begin-launch to its end-launch; solve_attempt stages the
// levels and picks the driver; tsba_solve owns the token, the clock and the pose-only retry.  DESIGN.md, "Pass boundaries".
struct PassCarry {                                // what a pass hands to the next one
    const bool per_step;                          // this attempt keeps the launch-per-step schedules (tsba_debug_options.pass_launches, or the pose-only retry)
    bool log_pending = false;                     // the pass before left its final state in W.st only: the next begin-launch (or k_solve_end) copies it to st_log
    int ms_ahead = -1;                            // the pass whose mu / sigma the previous pass's k_pass_end has computed
    bool clear_part = false;                      // a pass of this solve may begin with k_pass_begin, which expects the participation arrays clear
};
static bool pose_path(const Ctx *c) { return c->pose_only && !is_multi(c); }
// The kernels of an LM iteration return at once when the pass has converged, but each still costs a launch (~4 us):
// the host reads the pinned progress word and stays at most two iterations ahead of the device -- no API call, no
// synchronisation -- so a pass that converges early wastes two iterations of empty launches instead of all the rest.
static bool converged(const Ctx *c, int it) {
    if (!c->hprog || is_multi(c)) return false;
    const auto tw = std::chrono::steady_clock::now();
    for (int spin = 0;; spin++) {
        const unsigned long long w = *(volatile unsigned long long *)c->hprog;
        if ((unsigned int)(w >> 32) == c->W.pass_seq) { if (w & 1) return true; if ((int)((w & 0xffffffffu) >> 1) + 2 > it) break; }
        else if (it < 2) break;                              // the device has not reached this pass yet
        PlanPool::cpu_relax();
        if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - tw > std::chrono::seconds(2)) break;   // never hang on it
    }
    return false;
}
// level l on the device and visible to the compute stream: staged now if the upload left it (one-shot call on a small window: its plan is ready or nearly so), its event waited for if it went over the copy stream
static int level_ready(Ctx *c, int l) {
    if (!c->lev_built[l]) {
        if (!c->stage_p) { set_err(c, "level not staged"); return TSBA_ERR_STATE; }
        c->stage_async = true; const int rc = stage_level(c, c->stage_p, l, nullptr, nullptr); c->stage_async = false; if (rc) return rc; }
    if (c->lev_wait[l]) { hipStreamWaitEvent(c->stream, c->ev_stage[l], 0); c->lev_wait[l] = 0; }
    return TSBA_OK;
}
static void record_cov(Ctx *c, int ps) { if (c->cov_text >= 0 && c->cov_text < c->n_text && ps < TSBA_MAX_LEVELS) LAUNCHK(k_record_vtx, dim3(1), dim3(64), 0, c->stream, c->W, c->cov_text, c->cov_log + 6*ps); }
// PoseOptim (tsba_pose.h): k_pose_begin | the pass's LM steps in one launch (k_pose_pass) where its workgroups are all resident at once, otherwise a launch per step (k_pose_iter) | k_outlier with the workgroup that installs the pass's result
static int pose_pass(Ctx *c, int ps, PassCarry &carry) {
    const tsba_options &o = c->opt; const LevelDev &D = c->lev[o.levels[ps]]; const int G = pose_grid(D);
    const bool one_launch = !carry.per_step && grid_resident(c, (const void *)k_pose_pass, POSE_WG, 0, G);
    c->W.hprog = c->hprog; c->W.pass_seq = ++c->pass_seq;                 // (k_pose_begin: k_pass_reset + k_participation + k_gauge + k_musigma in one launch)
    LAUNCHK(k_pose_begin, dim3(D.n_tg + 1), dim3(MS_THREADS), 0, c->stream, c->W, D, o.initial_radius, o.its[ps], (const uint8_t *)c->kf_initial,
            one_launch ? c->W.ppart : (double *)nullptr, 3*28*G, carry.log_pending ? c->st_log + ps - 1 : (LmState *)nullptr);
    int k_last = -1;                                     // (k_pose_pass leaves the final state in pst[0])
    if (one_launch) LAUNCHK(k_pose_pass, dim3(G), dim3(POSE_WG), 0, c->stream, c->W, D, o, G, o.its[ps]);
    else {
        LAUNCHK(k_pose_iter, dim3(G), dim3(POSE_WG), 0, c->stream, c->W, D, o, -1, G);
        for (int k = 0; k <= o.its[ps]; k++) {           // launch k decides trial k - 1 and prepares trial k
            if (k >= 1 && converged(c, k - 1)) break;
            LAUNCHK(k_pose_iter, dim3(G), dim3(POSE_WG), 0, c->stream, c->W, D, o, k, G); k_last = k;
        }
        if (k_last < 0) k_last = 0;
    }
    // outlier pass + installation of the pass's result (one extra workgroup) in one launch
    LAUNCHK(k_outlier, dim3((D.n_sc + 63)/64 + D.n_tg + 1), dim3(64), 0, c->stream, c->W, D, o.chi2_mono[ps], o.chi2_text[ps],
                       o.text_bad_ratio, o.outlier_scene, o.outlier_text, (const PoseState *)(c->W.pst + ((k_last + 1) & 1)));
    carry.log_pending = true;                            // (kept by the next pass's k_pose_begin, or by k_solve_end)
    return stage_ahead(c, ps);                           // (one-shot calls: the later passes' levels, over the copy stream while this pass runs)
}
// the LM trials of a window's or a map's pass behind its begin-launch: the first linearisation, up to its[ps] trials, and (fused_decisions) the decision on the last one
// end_decides (window_pass): where the trials' k_mid launches carry the decision block, the last trial's decision is left to a workgroup of k_pass_end (*end_decides = true)
static int lm_trials(Ctx *c, const LevelDev &D, int ps, bool fuse_first, bool *end_decides = nullptr) {
    launch_linearize(c, D, 0, fuse_first); int n_trials = 0;
    for (int it = 0; it < c->opt.its[ps]; it++) {
        if (converged(c, it) && !(fuse_first && n_trials == 0)) break;
        launch_step(c, D, n_trials > 0, fuse_first && n_trials == 0); n_trials++;
        if (it >= 1) { const int rc = stage_ahead(c, ps); if (rc) return rc; }      // (with two iterations queued the device does not run dry while the host stages)
    }
    if (n_trials > 0 && fused_decisions(c, D)) {
        if (end_decides && decision_in_mid(c, D) && production_launches(c)) *end_decides = true;
        else launch_decide(c, D);
    }
    return TSBA_OK;
}
// windows on one GPU (window_fast): k_pass_begin | trials, the first one's assembly doing k_postlin's work | k_pass_end (tsba_kernels_pass.h)
static int window_pass(Ctx *c, int ps, PassCarry &carry) {
    const tsba_options &o = c->opt; const LevelDev &D = c->lev[o.levels[ps]];
    // The participation arrays are clear (k_reset_state / the last pass's end); the text observations' mu / sigma are there already if the last pass's k_pass_end computed them for this level
    c->cur_bw_rows = D.bw_rows; c->S_stale = true; c->x_pass = 0;
    c->W.hprog = c->hprog; c->W.pass_seq = ++c->pass_seq; c->W.trace_pass = ps;
    // (at most PB_WG workgroups walk k_participation's npb blocks: every arrival at the ticket is a device-wide fence and an atomic on one word -- 30 - 40 ns each, one after the other: tools/ticket_bench.hip)
    const int npb = (D.n_sc + 255)/256 + (D.n_tg + 3)/4, nwg = std::min(npb, PB_WG), n_ms = carry.ms_ahead == ps ? 0 : D.n_tg;
    LAUNCHK(k_pass_begin, dim3(nwg + n_ms), dim3(MS_THREADS), 0, c->stream, c->W, D, o.initial_radius, o.its[ps], (const uint8_t *)c->kf_initial, o.state,
                       npb, nwg, n_ms, carry.log_pending ? c->st_log + ps - 1 : (LmState *)nullptr, c->ticket);
    // k_postlin (the first linearisation's scaling, cost, gradient test: 8.6 us of one workgroup) inside the first trial's assembly
    bool end_decides = false;
    int rc = lm_trials(c, D, ps, o.its[ps] > 0 && c->dbg.trial_launches != 3, &end_decides); if (rc) return rc;
    // the outlier pass, the NEXT pass's mu / sigma (when its level is on the device already) and the clearing of the participation arrays in one launch
    const int nb_out = (o.outlier_scene || o.outlier_text) && D.n_sc + D.n_tg > 0 ? (D.n_sc + 63)/64 + D.n_tg : 0, ln = ps + 1 < o.n_passes ? o.levels[ps + 1] : -1;
    const LevelDev *Dn = ln >= 0 && c->lev_built[ln] && window_fast(c, c->lev[ln], carry.per_step) && c->lev[ln].n_tg > 0 ? &c->lev[ln] : nullptr;
    if (Dn) { rc = level_ready(c, ln); if (rc) return rc; }      // (staged over the copy stream during this pass's trials: long since there)
    const int n_msn = Dn ? Dn->n_tg : 0;
    PassDec pd{0, 0, 0, tsba_options{}};                 // (+ the workgroup of the last trial's decision, in front: k_decide's arguments)
    if (end_decides) { int nb_pt, nb_tx, nb_pr; mid_blocks(c, D, nb_pt, nb_tx, nb_pr);
        pd = PassDec{1, back_blocks_pt(c->n_pt) + back_blocks_tx(c->n_text) + (c->n_kf + 255)/256, nb_pt + nb_tx + nb_pr, c->opt}; }
    LAUNCHK(k_pass_end, dim3(pd.on + (nb_out + 3)/4 + n_msn + 1), dim3(MS_THREADS), 0, c->stream, c->W, D, Dn ? *Dn : D, nb_out, n_msn, c->musig2[c->musig_sel ^ 1],
                       o.chi2_mono[ps], o.chi2_text[ps], o.text_bad_ratio, o.outlier_scene, o.outlier_text, pd);
    if (Dn) { c->musig_sel ^= 1; c->W.musig = c->musig2[c->musig_sel]; carry.ms_ahead = ps + 1; }
    record_cov(c, ps);
    carry.log_pending = true;                            // (kept by the next pass's k_pass_begin, or by k_solve_end)
    return TSBA_OK;
}
// maps, sharded runs, pass_launches = 1: launch_pass_init | trials | k_outlier, the state's copy to st_log, the participation arrays' clearing
static int generic_pass(Ctx *c, int ps, PassCarry &carry) {
    const tsba_options &o = c->opt; const LevelDev &D = c->lev[o.levels[ps]];
    if (carry.log_pending) { CK(hipMemcpyAsync(c->st_log + ps - 1, c->W.st, sizeof(LmState), hipMemcpyDeviceToDevice, c->stream)); carry.log_pending = false; }
    launch_pass_init(c, D, ps);
    const int rc = lm_trials(c, D, ps, false); if (rc) return rc;
    if ((o.outlier_scene || o.outlier_text) && D.n_sc + D.n_tg > 0)
        LAUNCHK(k_outlier, dim3((D.n_sc + 63)/64 + D.n_tg), dim3(64), 0, c->stream, c->W, D, o.chi2_mono[ps], o.chi2_text[ps], o.text_bad_ratio, o.outlier_scene, o.outlier_text, (const PoseState *)nullptr);
    record_cov(c, ps);
    CK(hipMemcpyAsync(c->st_log + ps, c->W.st, sizeof(LmState), hipMemcpyDeviceToDevice, c->stream));
    if (carry.clear_part) LAUNCHK(k_part_clear, dim3(8), dim3(256), 0, c->stream, c->W);
    return TSBA_OK;
}
// the report of a finished attempt out of the pinned block k_solve_end wrote: the passes' final states, 8 ints of conjugate-gradient counters, the give-up count
static void fill_report(Ctx *c, tsba_report *r) {
    const tsba_options &o = c->opt; const int *pcg_host = (const int *)(c->st_host + TSBA_MAX_LEVELS);
    r->n_passes = o.n_passes; long long prev_lin = 0, prev_cost = 0;
    for (int ps = 0; ps < o.n_passes; ps++) {
        const LmState &s = c->st_host[ps];
        r->iters[ps] = s.it; r->accepted[ps] = s.accepted; r->termination[ps] = s.term;
        r->cost0[ps] = s.cost0; r->cost1[ps] = s.x_cost; r->n_sblock[ps] = s.ns_active; r->n_tblock[ps] = s.nt_active;
        r->n_bad_scene[ps] = s.n_bad_scene; r->n_bad_tfeat[ps] = s.n_bad_tfeat; r->n_bad_text[ps] = s.n_bad_text;
        r->n_resid_evals += ((s.n_lin - prev_lin) + (s.n_cost - prev_cost))*(2LL*s.ns_active + 8LL*s.nt_active);
        prev_lin = s.n_lin; prev_cost = s.n_cost;
        if (s.term == 5) r->status = TSBA_ERR_NUMERIC;
    }
    int use_lds; solve_lds_bytes(c, &use_lds); const LevelDev &Dl = c->lev[o.levels[o.n_passes - 1]];
    r->solver_path = pose_path(c) ? TSBA_SOLVER_POSE : use_lds ? TSBA_SOLVER_LDS
        : Dl.far_B > 0 ? (Dl.n_wb > 0 && ms_available(c) && c->dbg.far_solver != 3 ? TSBA_SOLVER_BAND_LOWRANK : TSBA_SOLVER_BAND_PCG)
        : !c->band_stream ? TSBA_SOLVER_DENSE : c->band_parts <= 1 ? TSBA_SOLVER_BAND : c->W.ring ? TSBA_SOLVER_RING : c->sep_cr ? TSBA_SOLVER_BAND_CR : TSBA_SOLVER_BAND_PART;
    r->poll_timeouts = (int32_t)((const unsigned int *)pcg_host)[8];
    if (c->far_B > 0) { r->pcg_iterations = pcg_host[0]; r->pcg_systems = pcg_host[1]; r->pcg_max_iterations = pcg_host[2]; r->pcg_unconverged = pcg_host[3]; r->pcg_stagnated = pcg_host[4]; }
}
static int enqueue_pack(Ctx *c);
// one run of the uploaded problem from its start point, into a zeroed report
static int solve_attempt(Ctx *c, tsba_report *r, bool per_step) {
    const tsba_options &o = c->opt; int rc = reset_state(c); if (rc) return rc;
    if (c->far_B > 0) hipMemsetAsync(c->W.pc_stat, 0, 8*sizeof(int), c->stream);
    PassCarry carry{per_step};
    for (int ps = 0; ps < o.n_passes; ps++) { const int l = o.levels[ps];
        if (c->lev_built[l] ? window_fast(c, c->lev[l], per_step) : window_fast_ctx(c, per_step)) carry.clear_part = true; }
    for (int ps = 0; ps < o.n_passes; ps++) {
        rc = level_ready(c, o.levels[ps]); if (rc) return rc;
        rc = pose_path(c) ? pose_pass(c, ps, carry) : window_fast(c, c->lev[o.levels[ps]], per_step) ? window_pass(c, ps, carry) : generic_pass(c, ps, carry); if (rc) return rc;
    }
    const int nl = c->n_pt + 3*c->n_text;
    if (c->world > 1 && nl > 0) {                 // every landmark was optimised by its owner only
        LAUNCHK(k_delta_multi, dim3((nl + 255)/256), dim3(256), 0, c->stream, c->W, (const double *)c->rho0, (const double *)c->theta0, 0);
        if (c->n_pt) allreduce(c, c->W.dl_pt, c->n_pt, ncclDouble, ncclSum);
        if (c->n_text) allreduce(c, c->W.dl_tx, 3*(size_t)c->n_text, ncclDouble, ncclSum);
        LAUNCHK(k_delta_multi, dim3((nl + 255)/256), dim3(256), 0, c->stream, c->W, (const double *)c->rho0, (const double *)c->theta0, 1);
    }
    // the passes' final states straight into pinned host memory (a kernel's stores: no copy engine, no staging), the give-up count behind the 8 ints of pc_stat
    LAUNCHK(k_solve_end, dim3(1), dim3(64), 0, c->stream, c->W, c->st_log, o.n_passes, carry.log_pending ? 1 : 0, c->st_host, (unsigned int *)(c->st_host + TSBA_MAX_LEVELS) + 8);
    if (c->far_B > 0) CK(hipMemcpyAsync(c->st_host + TSBA_MAX_LEVELS, c->W.pc_stat, 8*sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (c->pack_in_solve) { rc = enqueue_pack(c); if (rc) return rc; }
    CK(hipStreamSynchronize(c->stream)); CK(hipGetLastError());
    c->packed = c->pack_in_solve;
    if (!c->err.empty() && c->err.rfind("ncclAllReduce", 0) == 0) return TSBA_ERR_COMM;
    fill_report(c, r);
    return TSBA_OK;
}
int tsba_solve(void *ctx, tsba_report *r) {
    Ctx *c = (Ctx *)ctx; if (!c || !r) return TSBA_ERR_ARG;
    c->packed = false;
    if (!c->uploaded) { set_err(c, "no problem uploaded"); return TSBA_ERR_STATE; }
    hipSetDevice(c->device);
    memset(r, 0, sizeof(*r));
    { int rca = set_solver_attrs(c); if (rca) return rca; }
    struct Poison { Poison(int v) { g_lds_poison = v; } ~Poison() { g_lds_poison = 0; } } poison(c->dbg.lds_poison);
    struct Token { Ctx *c; Token(Ctx *c_) : c(c_) { if (c->lgroup) { c->in_solve = true; c->lgroup->gpu_token.lock(); c->has_token = true; } }
                   ~Token() { if (c->lgroup) { c->in_solve = false; if (c->has_token) { hipStreamSynchronize(c->stream); c->has_token = false; c->lgroup->gpu_token.unlock(); } } } } token(c);
    const auto t0 = std::chrono::steady_clock::now();
    const bool drill = pose_path(c) && c->dbg.pass_launches == 2;      // (tsba_debug.h: the first attempt runs as in production and counts as abandoned)
    const bool per_step = c->dbg.pass_launches != 0 && !drill;
    int rc = solve_attempt(c, r, per_step); if (rc) return rc;
    if (drill) r->poll_timeouts += 1;
    // PoseOptim in one launch per pass (k_pose_pass): every workgroup keeps the LM state redundantly and assumes that all of them read the same polled sums -- a poll that ran
    // into its bound in ONE workgroup (a dispatch stall of ~100 ms beside another context) would let the copies part silently.  A give-up anywhere during such a
    // solve: the answer is not used, the solve runs again from its start point with a launch per LM step (k_pose_iter: no workgroup waits for another)
    if (pose_path(c) && !per_step && r->poll_timeouts != 0) {
        const int32_t gave_up = r->poll_timeouts;
        memset(r, 0, sizeof(*r));
        rc = solve_attempt(c, r, true); if (rc) return rc;
        r->poll_timeouts += gave_up;                     // (reported: the caller sees that the first attempt was abandoned)
    }
    r->t_solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return TSBA_OK;
}

// the results of a solve -- LM state, the current poses / inverse depths / plane parameters, the three flag arrays -- gathered into one block on the
// device (which of the two parameter buffers is current is device-side state) and brought over by ONE copy into pinned memory: seven synchronous
// copies into pageable memory, the first of them only to learn an index, were 0.22 ms of a 3.8 ms local-BA call
struct DlLayout { size_t o_pose, o_rho, o_theta, o_sg, o_to, o_tf, total; };        // what the kernel gets: the spans' offsets
struct DlSpans { Span<LmState> st; Span<double> pose, rho, theta; Span<uint8_t> sg, to, tf; DlLayout dev; };
static DlSpans dl_layout(const Ctx *c) {
    // [LmState | pose | rho | theta | sgood | tobs_good | tfgood]
    Layout L(16); DlSpans S;
    S.st = L.take<LmState>(1); S.pose = L.take<double>(7*(size_t)c->n_kf); S.rho = L.take<double>((size_t)c->n_pt); S.theta = L.take<double>(3*(size_t)c->n_text);
    S.sg = L.take<uint8_t>((size_t)c->n_sgood); S.to = L.take<uint8_t>((size_t)c->n_tobs); S.tf = L.take<uint8_t>((size_t)c->n_tfgood);
    S.dev = {S.pose.off, S.rho.off, S.theta.off, S.sg.off, S.to.off, S.tf.off, L.mark()};
    return S;
}
__global__ __launch_bounds__(256) void k_pack_results(Work W, DlLayout L, unsigned char *out, int n_kf, int n_pt, int n_text, int n_sg, int n_to, int n_tf) {
    const LmState *st = W.st; const int cur = st->cur & 1;
    const size_t t = (size_t)blockIdx.x*256 + threadIdx.x, nt = (size_t)gridDim.x*256;
    double *o_pose = (double *)(out + L.o_pose), *o_rho = (double *)(out + L.o_rho), *o_theta = (double *)(out + L.o_theta);
    if (t < sizeof(LmState)/4) ((int *)out)[t] = ((const int *)st)[t];
    for (size_t k = t; k < 7*(size_t)n_kf; k += nt) o_pose[k] = W.pose[cur][k];
    for (size_t k = t; k < (size_t)n_pt; k += nt) o_rho[k] = W.rho[cur][k];
    for (size_t k = t; k < 3*(size_t)n_text; k += nt) o_theta[k] = W.theta[cur][k];
    for (size_t k = t; k < (size_t)n_sg; k += nt) out[L.o_sg + k] = W.sgood[k];
    for (size_t k = t; k < (size_t)n_to; k += nt) out[L.o_to + k] = W.tobs_good[k];
    for (size_t k = t; k < (size_t)n_tf; k += nt) out[L.o_tf + k] = W.tfgood[k];
}
// The one-shot entry points (round 6) pack the results INSIDE the solve, behind its last kernel and before its one synchronisation -- small blocks (a pose-only
// call: 5 KB, a window: 60 KB) as the kernel's own stores into pinned host memory, larger ones through the device block and one copy: tsba_download then
// only copies out of the pinned block (no launch, no second synchronisation: 0.06 ms of a 0.66 ms tsba_pose_optim call).
#define TSBA_PACK_DIRECT_MAX ((size_t)256 << 10)
static int enqueue_pack(Ctx *c) {                 // (no synchronisation: the caller's)
    const DlLayout L = dl_layout(c).dev;
    if (int rc = reserve(c, c->dl_dev, "results block", L.total, L.total + L.total/4)) return rc;
    if (int rc = reserve(c, c->dl_host, "results block (pinned)", L.total, L.total + L.total/4)) return rc;
    const bool direct = L.total <= TSBA_PACK_DIRECT_MAX;
    const size_t work = std::max<size_t>({7*(size_t)c->n_kf, (size_t)c->n_pt, 3*(size_t)c->n_text, (size_t)c->n_sgood, (size_t)c->n_tobs, (size_t)c->n_tfgood, 64});
    LAUNCHK(k_pack_results, dim3((unsigned)std::min<size_t>(direct ? 64 : 1024, (work + 255)/256)), dim3(256), 0, c->stream, c->W, L, direct ? c->dl_host.as<unsigned char>() : c->dl_dev.as<unsigned char>(), c->n_kf, c->n_pt, c->n_text, c->n_sgood, c->n_tobs, c->n_tfgood);
    if (!direct) CK(hipMemcpyAsync(c->dl_host.as(), c->dl_dev.as(), L.total, hipMemcpyDeviceToHost, c->stream));
    return TSBA_OK;
}
int tsba_download(void *ctx, tsba_problem *p) {
    Ctx *c = (Ctx *)ctx; if (!c || !p) return TSBA_ERR_ARG;
    if (!c->uploaded) { set_err(c, "no problem uploaded"); return TSBA_ERR_STATE; }
    hipSetDevice(c->device);
    static_assert(sizeof(LmState) % 4 == 0, "LmState is copied as words");
    const DlSpans S = dl_layout(c);
    if (c->packed) c->packed = false;             // (the solve that has just ended left the block in pinned memory)
    else { int rc = enqueue_pack(c); if (rc) return rc;
        CK(hipStreamSynchronize(c->stream)); CK(hipGetLastError()); }
    const void *h = c->dl_host.as();
    S.pose.get(h, p->pose); S.rho.get(h, p->rho); S.theta.get(h, p->theta); S.sg.get(h, p->sgood); S.to.get(h, p->tobs_good); S.tf.get(h, p->tfgood);
    return TSBA_OK;
}

static int one_shot(void *ctx, tsba_problem *p, const tsba_options *o, tsba_report *r) {
    auto t0 = std::chrono::steady_clock::now();
    int rc = upload_impl(ctx, p, o, true); if (rc) return rc;
    auto t1 = std::chrono::steady_clock::now();
    ((Ctx *)ctx)->pack_in_solve = true;
    rc = tsba_solve(ctx, r);
    ((Ctx *)ctx)->pack_in_solve = false;
    { Ctx *c = (Ctx *)ctx; join_planners(c); c->stage_p = nullptr;      // (*p is the caller's: nothing may be staged from it after this call)
      for (int l = 0; l < (int)c->lev_planned.size(); l++) if (c->lev_planned[l] && !c->lev_built[l]) c->uploaded = false; }   // a failed solve left a level unstaged: upload again before anything else
    if (rc) return rc;
    auto t2 = std::chrono::steady_clock::now();
    rc = tsba_download(ctx, p); if (rc) return rc;
    auto t3 = std::chrono::steady_clock::now();
    r->t_upload_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    r->t_download_ms = std::chrono::duration<double, std::milli>(t3 - t2).count();
    return r->status;
}
int tsba_local_ba(void *ctx, tsba_problem *p, const tsba_options *o, tsba_report *r) { return one_shot(ctx, p, o, r); }
int tsba_pose_optim(void *ctx, tsba_problem *p, const tsba_options *o, tsba_report *r) {
    if (p && p->n_kf != 1) { if (ctx) set_err((Ctx *)ctx, "tsba_pose_optim needs n_kf == 1"); return TSBA_ERR_ARG; }
    return one_shot(ctx, p, o, r);
}
int tsba_global_ba(void *ctx, tsba_problem *p, const tsba_options *o, tsba_report *r) { return one_shot(ctx, p, o, r); }
// Information matrix of theta = V of the linearisation at the end of a pass (undamped, loss-corrected J^T J).  The reference runs ceres::Covariance after
// EVERY pyramid pass and keeps the last one that succeeds (optimizer.cc:2219-2238: thetaVariance is only overwritten when Compute returns true): the passes are
// tried from the last to the first.  A pass fails when V is not positive definite or its reciprocal condition number is below 1e-14 (Ceres'
// min_reciprocal_condition_number; recalled, oracle/RECALLED.md).  No pass succeeds: as the reference (PyrThetaOptim still returns true,
// optimizer.cc:2224-2241) not an error, cov[] untouched.  Vall: [passes][6] (xx xy xz yy yz zz).  Returns cov_valid.
static int theta_cov_select(const double *Vall, int n_passes, double cov[9]) {
    for (int ps = std::min(n_passes, TSBA_MAX_LEVELS) - 1; ps >= 0; ps--) {
        const double *V = Vall + 6*ps;
        const double a = V[0], b = V[1], cc = V[2], e = V[3], f = V[4], i = V[5];
        const double A = e*i - f*f, B = -(b*i - cc*f), C = b*f - cc*e, det = a*A + b*B + cc*C;
        if (!(det > 0.0) || !(a > 0.0) || !(a*e - b*b > 0.0)) continue;
        // eigenvalues of the symmetric 3x3 (trigonometric form): reciprocal condition number
        const double q = (a + e + i)/3.0, p1 = b*b + cc*cc + f*f, p2 = (a - q)*(a - q) + (e - q)*(e - q) + (i - q)*(i - q) + 2.0*p1, pp = sqrt(p2/6.0);
        double lmin = q, lmax = q;
        if (pp > 0.0) { const double ip = 1.0/pp, b00 = (a - q)*ip, b01 = b*ip, b02 = cc*ip, b11 = (e - q)*ip, b12 = f*ip, b22 = (i - q)*ip;
            double hr = 0.5*(b00*(b11*b22 - b12*b12) - b01*(b01*b22 - b12*b02) + b02*(b01*b12 - b11*b02));
            hr = hr < -1.0 ? -1.0 : (hr > 1.0 ? 1.0 : hr);
            const double phi = acos(hr)/3.0; lmax = q + 2.0*pp*cos(phi); lmin = q + 2.0*pp*cos(phi + 2.0943951023931953); }
        if (!(lmin > 1e-14*lmax)) continue;
        const double id = 1.0/det;
        cov[0] = A*id; cov[1] = B*id; cov[2] = C*id; cov[3] = B*id; cov[4] = (a*i - cc*cc)*id; cov[5] = -(a*f - b*cc)*id;
        cov[6] = C*id; cov[7] = cov[5]; cov[8] = (a*e - b*b)*id;
        return 1;
    }
    return 0;
}
int tsba_theta_optim(void *ctx, tsba_problem *p, const tsba_options *o, int text, double cov[9], tsba_report *r) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !p || !o || !cov || !r || text < 0 || text >= p->n_text) return TSBA_ERR_ARG;
    c->cov_text = text;
    int rc = one_shot(ctx, p, o, r);
    c->cov_text = -1;
    if (rc) return rc;
    double Vall[6*TSBA_MAX_LEVELS];
    CK(hipMemcpy(Vall, c->cov_log, sizeof(Vall), hipMemcpyDeviceToHost));
    r->cov_valid = theta_cov_select(Vall, o->n_passes, cov);
    return TSBA_OK;
}

// optimizer::ThetaOptimMultiFs for n independent planes in one launch (k_theta_batch, tsba_theta.h).  Host side: validate every problem, pack every plane's
// header, frames, features and the deduplicated host image planes into one pinned block (one host-to-device copy), one launch, one copy of the output
// records back, the covariance rule of tsba_theta_optim per plane.
static int theta_batch_check(Ctx *c, tsba_problem *const *probs, int n, const tsba_options *o) {
    auto bad = [&](int i, const std::string &why) { set_err(c, "tsba_theta_optim_batch: " + (i >= 0 ? "problem " + std::to_string(i) + ": " : std::string()) + why); return TSBA_ERR_ARG; };
    if (o->use_text != 1 || o->filter_good != 0 || o->outlier_scene != 0 || o->outlier_text != 0)
        return bad(-1, "options need use_text = 1, filter_good = 0, outlier_scene = outlier_text = 0 (tsba_default_options_theta)");
    if (o->text_jacobian != 0) return bad(-1, "text_jacobian must be 0 (analytic)");
    if (o->n_passes < 1 || o->n_passes > TSBA_MAX_LEVELS) return bad(-1, "n_passes out of range");
    for (int ps = 0; ps < o->n_passes; ps++) if (o->levels[ps] < 0 || o->levels[ps] >= TSBA_MAX_LEVELS) return bad(-1, "options.levels out of range");
    for (int i = 0; i < n; i++) {
        const tsba_problem *p = probs[i];
        if (!p) return bad(i, "NULL problem");
        if (p->n_text != 1 || !p->theta || !p->text_host || !p->text_box_ray) return bad(i, "needs n_text == 1");
        if (p->n_kf < 1 || !p->pose || !p->kf_initial || p->text_host[0] < 0 || p->text_host[0] >= p->n_kf) return bad(i, "needs 0 <= text_host[0] < n_kf");
        if (p->n_pt != 0) return bad(i, "needs n_pt == 0");
        for (int l = 0; l < TSBA_MAX_LEVELS; l++) if (p->n_sobs[l] != 0) return bad(i, "needs n_sobs[l] == 0 at every level");
        for (int k = 0; k < p->n_kf; k++) if (p->kf_initial[k] != 1) return bad(i, "needs kf_initial[k] == 1 for every keyframe (all poses constant)");
        if (p->n_tobs < 0 || (p->n_tobs > 0 && (!p->tobs_kf || !p->tobs_text))) return bad(i, "bad text observations");
        for (int t = 0; t < p->n_tobs; t++) {
            if (p->tobs_text[t] != 0) return bad(i, "needs tobs_text[t] == 0");
            if (p->tobs_kf[t] < 0 || p->tobs_kf[t] >= p->n_kf) return bad(i, "tobs_kf out of range");
        }
        for (int ps = 0; ps < o->n_passes; ps++) {
            const int l = o->levels[ps];
            if (l >= p->n_levels) return bad(i, "level " + std::to_string(l) + " of the options does not exist");
            if (!p->img[l] || !image_dims_ok(p->img_w[l], p->img_h[l])) return bad(i, "missing image level or image side above TSBA_MAX_IMAGE_DIM (" + std::to_string(TSBA_MAX_IMAGE_DIM) + ")");
            if (!p->tfeat_off[l] || p->tfeat_off[l][0] != 0 || p->tfeat_off[l][1] < 0 || p->tfeat_off[l][1] > p->n_tfeat[l]
                || (p->tfeat_off[l][1] > 0 && (!p->tfeat_uv[l] || !p->tfeat_ref[l]))) return bad(i, "bad reference features");
            for (int t = 0; t < p->n_tobs; t++) if (!p->img[l][p->tobs_kf[t]]) return bad(i, "NULL image plane");
        }
    }
    return TSBA_OK;
}
int tsba_theta_optim_batch(void *ctx, tsba_problem *const *probs, int n, const tsba_options *o, double *cov, tsba_report *reps) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return TSBA_ERR_ARG;
    if (n < 0 || (n > 0 && (!probs || !o || !cov || !reps))) { set_err(c, "tsba_theta_optim_batch: bad arguments"); return TSBA_ERR_ARG; }
    if (n == 0) return TSBA_OK;
    int rc = theta_batch_check(c, probs, n, o); if (rc) return rc;
    hipSetDevice(c->device);
    auto t0 = std::chrono::steady_clock::now();
    // ---- the staged block: [headers | frames | feature uv | feature ref | image planes (each host plane once per call)]; behind it on the device: [scratch | output records]
    int n_obs = 0; size_t n_feat = 0;
    for (int i = 0; i < n; i++) { const tsba_problem *p = probs[i]; n_obs += p->n_tobs;
        for (int l = 0; l < p->n_levels && l < TSBA_MAX_LEVELS; l++) if (p->tfeat_off[l]) n_feat += (size_t)p->tfeat_off[l][1]; }
    Layout L(256);
    const auto a_hdr = L.take<ThHdr>((size_t)n); const auto a_obs = L.take<ThObs>((size_t)std::max(n_obs, 1));
    const auto a_uv = L.take<double>(2*std::max<size_t>(n_feat, 1)), a_ref = L.take<double>(8*std::max<size_t>(n_feat, 1));
    struct Plane { const uint8_t *src; Span<uint8_t> at; size_t end; };          // end: where the next plane begins (the gap up to it is zeroed)
    std::vector<Plane> planes;                                                  // host planes in first-use order
    std::map<const uint8_t *, size_t> seen;
    if (!o->img_on_device)
        for (int i = 0; i < n; i++) { const tsba_problem *p = probs[i];
            for (int ps = 0; ps < o->n_passes; ps++) { const int l = o->levels[ps];
                for (int t = 0; t < p->n_tobs; t++) { const uint8_t *src = p->img[l][p->tobs_kf[t]];
                    if (seen.count(src)) continue;
                    const auto a = L.take<uint8_t>((size_t)p->img_w[l]*p->img_h[l] + 2);                         // (+2: tap_fetch's 2-byte loads)
                    seen[src] = a.off; planes.push_back({src, a, L.mark()}); } } }
    const size_t staged = L.mark();
    const auto a_scr = L.take<double>((size_t)THETA_SCR*std::max(n_obs, 1)); const auto a_out = L.take<ThOut>((size_t)n);
    Layout Lo(256); const auto h_out = Lo.take<ThOut>((size_t)n);               // the output records in the pinned out block
    if ((rc = reserve(c, c->tb_host, "theta batch staging", staged, staged + staged/4))) return rc;
    if ((rc = reserve(c, c->tb_dev, "theta batch device block", L.mark(), L.mark() + L.mark()/4))) return rc;
    if ((rc = reserve(c, c->tb_out, "theta batch output records", h_out.bytes(), h_out.bytes() + h_out.bytes()/4))) return rc;
    unsigned char *hb = c->tb_host.as<unsigned char>(), *db = c->tb_dev.as<unsigned char>();
    ThHdr *hh = a_hdr.at(hb); ThObs *ho = a_obs.at(hb); double *huv = a_uv.at(hb), *href = a_ref.at(hb);
    int ob = 0; size_t fb = 0;
    for (int i = 0; i < n; i++) {
        const tsba_problem *p = probs[i]; ThHdr &H = hh[i];
        memset(&H, 0, sizeof(H));
        for (int k = 0; k < 4; k++) H.K[k] = p->K[k];
        for (int k = 0; k < 3; k++) H.theta[k] = p->theta[k];
        for (int k = 0; k < 7; k++) H.host[k] = p->pose[7*p->text_host[0] + k];
        for (int k = 0; k < 8; k++) H.box[k] = p->text_box_ray[k];
        H.n_obs = p->n_tobs; H.o_obs = ob;
        for (int t = 0; t < p->n_tobs; t++) { ThObs &O = ho[ob + t]; const int kf = p->tobs_kf[t];
            for (int k = 0; k < 7; k++) O.pose[k] = p->pose[7*kf + k];
            for (int l = 0; l < TSBA_MAX_LEVELS; l++) O.img[l] = nullptr; }
        for (int l = 0; l < p->n_levels && l < TSBA_MAX_LEVELS; l++) {
            const int nf = p->tfeat_off[l] ? p->tfeat_off[l][1] : 0;
            H.nf[l] = nf; H.o_feat[l] = (int)fb; H.w[l] = p->img_w[l]; H.h[l] = p->img_h[l];
            if (nf) { memcpy(huv + 2*fb, p->tfeat_uv[l], sizeof(double)*2*nf); memcpy(href + 8*fb, p->tfeat_ref[l], sizeof(double)*8*nf); }
            fb += nf;
        }
        for (int ps = 0; ps < o->n_passes; ps++) { const int l = o->levels[ps];
            for (int t = 0; t < p->n_tobs; t++) { const uint8_t *src = p->img[l][p->tobs_kf[t]];
                ho[ob + t].img[l] = o->img_on_device ? src : (const uint8_t *)(db + seen[src]); } }
        ob += p->n_tobs;
    }
    for (const Plane &P : planes) {                                // the image planes: a memcpy each into the pinned block (one copy to the device for all)
        const size_t len = P.at.n - 2;
        memcpy(P.at.at(hb), P.src, len); memset(P.at.at(hb) + len, 0, P.end - P.at.off - len);
    }
    CK(hipMemcpyAsync(db, hb, staged, hipMemcpyHostToDevice, c->stream));
    auto t1 = std::chrono::steady_clock::now();
    ThArgs A; A.hdr = a_hdr.at(db); A.obs = a_obs.at(db); A.fuv = a_uv.at(db); A.fref = a_ref.at(db);
    A.scr = a_scr.at(db); A.out = a_out.at(db);
    void (*const kern)(ThArgs, tsba_options) = k_theta_batch<THETA_WG>;
    LAUNCHK(kern, dim3(n), dim3(THETA_WG), 0, c->stream, A, *o);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(h_out.at(c->tb_out.as()), a_out.at(db), h_out.bytes(), hipMemcpyDeviceToHost, c->stream));
    CK(hipStreamSynchronize(c->stream));
    auto t2 = std::chrono::steady_clock::now();
    const ThOut *out = h_out.at(c->tb_out.as());
    for (int i = 0; i < n; i++) {
        tsba_problem *p = probs[i]; const ThOut &R = out[i]; tsba_report &r = reps[i];
        memset(&r, 0, sizeof(r));
        r.n_passes = o->n_passes; r.solver_path = TSBA_SOLVER_THETA;
        for (int ps = 0; ps < o->n_passes; ps++) {
            const int l = o->levels[ps]; const long long nt = (long long)p->n_tobs*(p->tfeat_off[l] ? p->tfeat_off[l][1] : 0);
            r.iters[ps] = R.iters[ps]; r.accepted[ps] = R.accepted[ps]; r.termination[ps] = R.term[ps];
            r.cost0[ps] = R.cost0[ps]; r.cost1[ps] = R.cost1[ps]; r.n_tblock[ps] = nt;
            r.n_resid_evals += R.evals[ps]*8LL*nt;
            if (R.term[ps] == 5) r.status = TSBA_ERR_NUMERIC;
        }
        for (int k = 0; k < 3; k++) p->theta[k] = R.theta[k];
        if (r.status == TSBA_OK) r.cov_valid = theta_cov_select(&R.V[0][0], o->n_passes, cov + 9*(size_t)i);     // (a failed solve, as tsba_theta_optim: cov untouched)
    }
    auto t3 = std::chrono::steady_clock::now();
    const double tu = std::chrono::duration<double, std::milli>(t1 - t0).count(), tsv = std::chrono::duration<double, std::milli>(t2 - t1).count(),
                 td = std::chrono::duration<double, std::milli>(t3 - t2).count();
    for (int i = 0; i < n; i++) { reps[i].t_upload_ms = tu; reps[i].t_solve_ms = tsv; reps[i].t_download_ms = td; }
    return TSBA_OK;
}

int tsba_eval(void *ctx, const tsba_problem *p, const tsba_options *o, int level,
              double *resid, double *jac, double *musigma, int64_t *ns_out, int64_t *nt_out) {
    Ctx *c = (Ctx *)ctx; if (!c) return TSBA_ERR_ARG;
    if (!p || level < 0 || level >= p->n_levels) return TSBA_ERR_ARG;
    tsba_options oo = *o; oo.n_passes = 1; oo.levels[0] = level;
    int rc = tsba_upload(ctx, p, &oo); if (rc) return rc;
    rc = reset_state(c); if (rc) return rc;
    const LevelDev &D = c->lev[level]; const HostPlan &H = c->hplan[level];
    launch_pass_init(c, D, 0);
    // reference block order: scene candidates by observation index, then text blocks by (tobs, feature)
    std::vector<int> out_idx(H.n_sc(), -1);
    { std::vector<int> by_obs(p->n_sobs[level], -1);
      for (int q = 0; q < H.n_sc(); q++) by_obs[H.sc_obs[q]] = q;
      int n = 0;
      for (int s = 0; s < p->n_sobs[level]; s++) { int q = by_obs[s]; if (q < 0) continue;
          if (oo.filter_good && !p->sgood[H.sc_flag[q]]) continue; out_idx[q] = n++; }
      *ns_out = n; }
    std::vector<int> bg, bf;
    for (int g = 0; g < H.n_tg(); g++) {
        int tb = H.tg_tobs[g], j = H.tg_text[g];
        if (oo.filter_good && !p->tobs_good[tb]) continue;
        for (int f = p->tfeat_off[level][j]; f < p->tfeat_off[level][j+1]; f++) {
            if (oo.filter_good && !p->tfgood[p->tobs_fgood_off[tb] + p->tfeat_raw[level][f]]) continue;
            bg.push_back(g); bf.push_back(f);
        }
    }
    *nt_out = (int64_t)bg.size();
    int64_t ns = *ns_out, nt = *nt_out;
    if (resid || jac) {
        const int *d_oi, *d_bg, *d_bf; double *d_r, *d_j = nullptr;
        rc = dev_upload_vec(c, &d_oi, out_idx); if (rc) return rc;
        rc = dev_upload_vec(c, &d_bg, bg); if (rc) return rc;
        rc = dev_upload_vec(c, &d_bf, bf); if (rc) return rc;
        rc = dev_alloc(c, &d_r, (size_t)(2*ns + 8*nt)); if (rc) return rc;
        if (jac) { rc = dev_alloc(c, &d_j, (size_t)(26*ns + 120*nt)); if (rc) return rc; }
        flush_run(c);                                  // staged uploads leave as one copy
        if (H.n_sc() > 0) LAUNCHK(k_eval_scene, dim3((H.n_sc() + 255)/256), dim3(256), 0, c->stream, c->W, D, d_oi, d_r, d_j);
        if (nt > 0) LAUNCHK(k_eval_text, dim3(((int)nt + 255)/256), dim3(256), 0, c->stream, c->W, D, (int)nt, d_bg, d_bf, (int)ns, d_r, d_j);
        CK(hipStreamSynchronize(c->stream)); CK(hipGetLastError());
        if (resid) CK(hipMemcpy(resid, d_r, sizeof(double)*(size_t)(2*ns + 8*nt), hipMemcpyDeviceToHost));
        if (jac) CK(hipMemcpy(jac, d_j, sizeof(double)*(size_t)(26*ns + 120*nt), hipMemcpyDeviceToHost));
    }
    CK(hipStreamSynchronize(c->stream));
    if (musigma && p->n_tobs) CK(hipMemcpy(musigma, c->W.musig, sizeof(double)*2*p->n_tobs, hipMemcpyDeviceToHost));
    return TSBA_OK;
}

#include "tsba_debug_abi.h"
} // extern "C"
static unsigned long long plan_checksum(const HostPlan &H) {           // over EVERY list of the plan
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](const std::vector<int32_t> &v) { for (int32_t x : v) { h ^= (unsigned int)x; h *= 1099511628211ull; } h ^= v.size(); h *= 1099511628211ull; };
    mix(H.sb_a); mix(H.sb_b); mix(H.sb_pt_off); mix(H.sb_pt_s1); mix(H.sb_pt_s2); mix(H.sb_pt_lm); mix(H.sb_tx_off); mix(H.sb_tx_s1); mix(H.sb_tx_s2); mix(H.sb_tx_lm);
    for (const std::vector<int32_t> *v : { &H.kf_order, &H.sc_obs, &H.sc_kf, &H.sc_pt, &H.sc_flag, &H.sc_slot, &H.pair_i, &H.pair_h, &H.pair_hpos, &H.pair_sc_off, &H.pair_tg_off, &H.pair_tg,
                                           &H.tg_tobs, &H.tg_kf, &H.tg_text, &H.tg_pair, &H.tg_slot, &H.pt_pose6, &H.pt_pair4, &H.tx_pair8, &H.tg_ppos, &H.pf_g, &H.pf_f, &H.tg_rec,
                                           &H.pls_off, &H.pslot_pose, &H.pslot_pair, &H.pslot_lm, &H.tls_off, &H.tslot_pose, &H.tslot_pair, &H.tslot_lm, &H.sb_pab, &H.sb_pba,
                                           &H.pose_t_off, &H.pose_t, &H.pose_h_off, &H.pose_h, &H.pose_ps_off, &H.pose_ps, &H.pose_ps_lm, &H.pose_ts_off, &H.pose_ts, &H.pose_ts_lm, &H.sb_rng }) mix(*v);
    if (H.far_B > 0) { h ^= (unsigned long long)H.far_B; h *= 1099511628211ull;
        for (const std::vector<int32_t> *v : { &H.far_a, &H.far_b, &H.far_off, &H.far_ent, &H.fb_id, &H.fb_pab, &H.fb_pba, &H.fb_pt_off, &H.fb_pt_s1, &H.fb_pt_s2, &H.fb_pt_lm, &H.fb_tx_off, &H.fb_tx_s1, &H.fb_tx_s2, &H.fb_tx_lm }) mix(*v); }
    for (double x : H.sc_uv) { unsigned long long u; memcpy(&u, &x, 8); h ^= u; h *= 1099511628211ull; }
    h ^= (unsigned long long)(H.bw_pose*4 + H.ring*2) + 8ull*(unsigned)H.ring_k0; h *= 1099511628211ull;
    return h;
}
extern "C" {
unsigned long long tsba_debug_plan_checksum(const tsba_problem *p, const tsba_options *o, int level, int threads) {
    if (!p || !o || level < 0 || level >= p->n_levels) return 0;
    const int saved = tsba_plan_threads; tsba_plan_threads = threads;
    HostPlan H; build_plan(p, o, level, H, false, true, tsba_plan_checksum_ring);
    tsba_plan_threads = saved;
    return plan_checksum(H);
}
// the plan of a single-frame problem (every landmark frozen) as build_plan_single_frame writes it down: the same checksum as tsba_debug_plan_checksum's; 0: not such a problem.
// recycled != 0: into a plan object that held the generic plan of the same problem's level 0 before
unsigned long long tsba_debug_plan_checksum_single_frame(const tsba_problem *p, const tsba_options *o, int level, int recycled) {
    if (!p || !o || level < 0 || level >= p->n_levels || !plan_is_single_frame(p, o)) return 0;
    HostPlan H; if (recycled) build_plan(p, o, 0, H);
    build_plan_single_frame(p, o, level, H);
    return plan_checksum(H);
}
// the plan of (p, o, level) built into a plan object that held the plan of (warm, ow, warm_level) before -- as a context does from call to call
unsigned long long tsba_debug_plan_checksum_recycled(const tsba_problem *warm, const tsba_options *ow, int warm_level, int warm_threads,
                                                     const tsba_problem *p, const tsba_options *o, int level, int threads) {
    if (!warm || !ow || !p || !o || level < 0 || level >= p->n_levels || warm_level < 0 || warm_level >= warm->n_levels) return 0;
    const int saved = tsba_plan_threads;
    HostPlan H;
    tsba_plan_threads = warm_threads; build_plan(warm, ow, warm_level, H, false, true, tsba_plan_checksum_ring);
    tsba_plan_threads = threads; build_plan(p, o, level, H, false, true, tsba_plan_checksum_ring);
    tsba_plan_threads = saved;
    return plan_checksum(H);
}
// host-only: the band + long-range split of the plan of `level` (tsba_plan.h: HostPlan::far_* / fb_*) when bands of up to far_max_blocks pose blocks are allowed.
// out[0] band of the preconditioner M in pose blocks (0: no split: ring, reordering or plain band), [1] 6x6 blocks of E (all ranks'), [2] those this rank
// contributes to, [3] the plan's band bound, [4] ring, [5] keyframes reordered, [6] checksum of the block positions (low 31 bits), [7] slot pairs of E, [8] keyframes touched by E when few enough for the low-rank correction (else 0).
// Checks what the split promises -- every block of M within the band, every slot pair of a landmark in exactly one of M / E, the positions of E
// sorted -- and returns TSBA_ERR_STATE if not.
int tsba_debug_plan_far(const tsba_problem *p, const tsba_options *o, int level, int far_max_blocks, int force, int ring_max_blocks, int32_t out[9]) {
    if (!p || !o || !out || level < 0 || level >= p->n_levels) return TSBA_ERR_ARG;
    HostPlan H; build_plan(p, o, level, H, false, true, ring_max_blocks, far_max_blocks, force != 0);
    int mine = 0; long long npairs = 0;
    if (H.far_B > 0) {
        for (int q = 0; q < H.n_sb(); q++) if (H.sb_b[q] - H.sb_a[q] > H.far_B) return TSBA_ERR_STATE;
        for (int q = 0; q < H.n_far(); q++) { if (H.far_a[q] >= H.far_b[q]) return TSBA_ERR_STATE;
            if (q > 0 && !(H.far_a[q-1] < H.far_a[q] || (H.far_a[q-1] == H.far_a[q] && H.far_b[q-1] < H.far_b[q]))) return TSBA_ERR_STATE;
            const bool has = H.fb_pt_off[q+1] > H.fb_pt_off[q] || H.fb_tx_off[q+1] > H.fb_tx_off[q] || H.fb_pab[q] >= 0 || H.fb_pba[q] >= 0; mine += has;
            for (int e = H.fb_pt_off[q]; e < H.fb_pt_off[q+1]; e++) if (H.pslot_pose[H.fb_pt_s1[e]] != H.far_a[q] || H.pslot_pose[H.fb_pt_s2[e]] != H.far_b[q] || H.pslot_lm[H.fb_pt_s1[e]] != H.pslot_lm[H.fb_pt_s2[e]]) return TSBA_ERR_STATE; }
        npairs = (long long)H.fb_pt_s1.size() + (long long)H.fb_tx_s1.size();
        // slot pairs with pose(s1) <= pose(s2): those of M + those of E = all of them
        long long all = 0; for (int j = 0; j < p->n_pt; j++) { const long long n = H.pls_off[j+1] - H.pls_off[j]; all += n*(n + 1)/2; }
        for (int j = 0; j < p->n_text; j++) { const long long n = H.tls_off[j+1] - H.tls_off[j]; all += n*(n + 1)/2; }
        if ((long long)H.sb_pt_s1.size() + (long long)H.sb_tx_s1.size() + npairs != all) return TSBA_ERR_STATE;
    }
    unsigned long long h = 1469598103934665603ull;
    for (const std::vector<int32_t> *v : { &H.far_a, &H.far_b, &H.far_off, &H.far_ent }) for (int32_t x : *v) { h ^= (unsigned int)x; h *= 1099511628211ull; }
    out[0] = H.far_B; out[1] = H.n_far(); out[2] = mine; out[3] = H.bw_pose; out[4] = H.ring; out[5] = H.kf_order.empty() ? 0 : 1; out[6] = (int32_t)(h & 0x7fffffffu);
    out[7] = (int32_t)npairs; out[8] = (int32_t)H.wb_kf.size();
    return TSBA_OK;
}
// host-only: does the plan of `level` take the ring path (one loop closure between the last and the first keyframes) when separators of up
// to ring_max_blocks pose blocks are allowed?  Returns 1 / 0 (< 0: error); *bw_pose = the band of the plan either way
int tsba_debug_plan_ring(const tsba_problem *p, const tsba_options *o, int level, int ring_max_blocks, int32_t *bw_pose) {
    if (!p || !o || !bw_pose || level < 0 || level >= p->n_levels) return TSBA_ERR_ARG;
    HostPlan H; build_plan(p, o, level, H, false, true, ring_max_blocks);
    *bw_pose = H.bw_pose;
    return H.ring ? 1 + 16*H.ring_k0 : 0;     // (the first keyframe of the loop in the upper bits: 0 = the whole trajectory)
}
void tsba_debug_bandp_part_ring(int nb, int B, int Pmax, int p, int *out5) { const BandpPart r = bandp_part_ring(nb - B, 0, B, Pmax, Pmax, p); out5[0] = r.P; out5[1] = r.a; out5[2] = r.b; out5[3] = r.has_left; out5[4] = r.has_right; }
// ring with a tail: nf free poses, the loop starts at free row row0; out8 = P, a, b, has_left, has_right, G, Pt, label of the left separator
void tsba_debug_bandp_part_ring2(int nf, int row0, int B, int Pmax, int Gmax, int p, int *out8) { const BandpPart r = bandp_part_ring(nf, row0, B, Pmax, Gmax, p);
    out8[0] = r.P; out8[1] = r.a; out8[2] = r.b; out8[3] = r.has_left; out8[4] = r.has_right; out8[5] = r.G; out8[6] = r.Pt; out8[7] = r.lblL; }
// the layout an upload would choose (tests/test_solver_layout.py).  A ring is taken as the plan builder makes one (tsba_plan.h): a band of 1 .. CR_SMAX / 6 pose
// blocks, a loop of at least four interiors of 3 B + 2 blocks and their separators
int tsba_debug_solver_layout(int n_kf, int bw_rows, int ring, int ring_k0, int multi, const tsba_debug_options *d, int32_t out[12]) {
    if (!out || n_kf < 1 || bw_rows < 0 || ring_k0 < 0 || ring_k0 >= n_kf) return TSBA_ERR_ARG;
    if (ring && (bw_rows < 6 || bw_rows > CR_SMAX || n_kf - ring_k0 < 4*(3*(bw_rows/6) + 2) + bw_rows/6)) return TSBA_ERR_ARG;
    const SolverLayout L = choose_solver_layout(n_kf, bw_rows, ring != 0, ring_k0, multi != 0, d ? *d : tsba_debug_options{});
    const int32_t v[12] = { L.use_lds, L.band, L.S_up, (int32_t)L.LDB, L.band_stream, L.P, L.sep_cr, L.partitioned, L.nsepb, L.ring, L.ring_G, L.xchg_wp };
    memcpy(out, v, sizeof(v)); return L.err;
}
int tsba_debug_sv_lmax(int n_kf, int B, int Pmax) { return sv_lmax_of(n_kf, B, Pmax); }      // the bound the solve phase sizes its LDS with (tests/test_band_partition.py)
void tsba_debug_bandp_part(int nb, int B, int Pmax, int p, int *out5) { const BandpPart r = bandp_part(nb, B, Pmax, p); out5[0] = r.P; out5[1] = r.a; out5[2] = r.b; out5[3] = r.has_left; out5[4] = r.has_right; }
long long tsba_debug_cr_blk_index(int mmax, int br, int bc) { return (long long)cr_blk_index(mmax, br, bc); }
long long tsba_debug_cr_pool_blocks(int mmax) { return (long long)cr_pool_blocks(mmax); }
int tsba_debug_stamps(void *ctx, long long *out64) {
    Ctx *c = (Ctx *)ctx; if (!c || !c->uploaded) return TSBA_ERR_STATE;
    hipSetDevice(c->device); hipStreamSynchronize(c->stream);
    return hipMemcpy(out64, c->W.dbg, 64*sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : TSBA_ERR_DEVICE;
}
#ifdef TSBA_SOLVE_STAMPS
int tsba_debug_step_stamps(void *ctx, long long *out128) {      // stamps build only: per factorisation step of the last k_solve_t launch
    Ctx *c = (Ctx *)ctx; if (!c) return TSBA_ERR_ARG;
    hipSetDevice(c->device); hipStreamSynchronize(c->stream);
    return hipMemcpyFromSymbol(out128, HIP_SYMBOL(ts_step_stamps), 128*sizeof(long long)) == hipSuccess ? 0 : TSBA_ERR_DEVICE;
}
#endif

// The library is loaded ONCE per process, under a lock -- and should be loaded (tsba_comm_load) before other host threads launch kernels: loading a HIP library registers its code
// objects with the runtime, and a kernel launch or hipFuncSetAttribute on another thread at that moment has been seen to fail ("invalid device function") and to crash (a segmentation
// fault inside another library's launch): the busy-context suite of round 6, test_multi_gpu_kernel_sequence_single_process beside an ORB extractor and a bundle adjustment looping on
// their own threads, once in about five runs (docs/ledger_r06.md 15.14).
static std::mutex g_rccl_mu; static void *g_rccl_so = nullptr; static std::string g_rccl_tried;
static void *rccl_handle() {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl_so) return g_rccl_so;
    // RCCL must sit on the SAME HIP runtime as this library: streams and device pointers do not cross runtimes.  A process can hold
    // two (a PyTorch wheel bundles its own libamdhip64 + librccl next to /opt/rocm's, and which one this library is bound to
    // depends on the load order), and a bare dlopen("librccl.so.1") returns whichever copy was loaded first.  So: find the
    // runtime our own HIP calls resolve to and take the librccl next to it, by full path.
    g_rccl_tried.clear();
    Dl_info di;
    if (dladdr((void *)&hipStreamSynchronize, &di) && di.dli_fname) {
        std::string dir(di.dli_fname); const size_t sl = dir.rfind('/'); dir = sl == std::string::npos ? std::string(".") : dir.substr(0, sl);
        for (const char *n : { "/librccl.so.1", "/librccl.so" }) {
            const std::string path = dir + n; g_rccl_tried += path + " ";
            g_rccl_so = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL); if (g_rccl_so) break; }
    }
    if (!g_rccl_so) for (const char *n : { "librccl.so.1", "librccl.so" }) { g_rccl_tried += std::string(n) + " "; g_rccl_so = dlopen(n, RTLD_NOW | RTLD_LOCAL); if (g_rccl_so) break; }
    return g_rccl_so;
}
static int load_rccl(Ctx *c) {
    if (c->rccl_so) return 0;
    c->rccl_so = rccl_handle();
    if (!c->rccl_so) { const char *e = dlerror(); set_err(c, std::string("dlopen(librccl) failed, tried: ") + g_rccl_tried + ": " + (e ? e : "")); return TSBA_ERR_COMM; }
    c->p_getid = (decltype(c->p_getid))dlsym(c->rccl_so, "ncclGetUniqueId");
    c->p_init = (decltype(c->p_init))dlsym(c->rccl_so, "ncclCommInitRank");
    c->p_allreduce = (decltype(c->p_allreduce))dlsym(c->rccl_so, "ncclAllReduce");
    c->p_destroy = (decltype(c->p_destroy))dlsym(c->rccl_so, "ncclCommDestroy");
    c->p_errstr = (decltype(c->p_errstr))dlsym(c->rccl_so, "ncclGetErrorString");
    c->p_count = (decltype(c->p_count))dlsym(c->rccl_so, "ncclCommCount");
    if (!c->p_getid || !c->p_init || !c->p_allreduce || !c->p_destroy || !c->p_errstr) { set_err(c, "librccl: missing symbols"); return TSBA_ERR_COMM; }
    return 0;
}
int tsba_comm_load(void) { return rccl_handle() ? TSBA_OK : TSBA_ERR_COMM; }
int tsba_comm_unique_id(void *ctx, void *id128) {
    Ctx *c = (Ctx *)ctx; if (!c || !id128) return TSBA_ERR_ARG;
    int rc = load_rccl(c); if (rc) return rc;
    ncclUniqueId id;
    ncclResult_t r = c->p_getid(&id);
    if (r != ncclSuccess) { set_err(c, std::string("ncclGetUniqueId: ") + c->p_errstr(r)); return TSBA_ERR_COMM; }
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    memcpy(id128, &id, 128);
    return TSBA_OK;
}
void *tsba_local_group_create(int world) {
    if (world < 1) return nullptr;
    LocalGroup *G = new LocalGroup(); G->world = world; G->stage.resize(world); return G;
}
void tsba_local_group_destroy(void *group) {
    LocalGroup *G = (LocalGroup *)group; if (!G) return;
    G->fail();
    for (Ctx *m : G->members) if (m && m->lgroup == G) { m->lgroup = nullptr; m->rank = 0; m->world = 1; m->uploaded = false; }   // (a resident problem was sharded for the group)
    delete G;
}
int tsba_comm_init_local(void *ctx, void *group, int rank, int world) {
    Ctx *c = (Ctx *)ctx; LocalGroup *G = (LocalGroup *)group;
    if (!c || !G || world != G->world || rank < 0 || rank >= world) return TSBA_ERR_ARG;
    hipSetDevice(c->device);
    free_problem(c);                               // any resident problem was sharded for the old world size
    c->lgroup = G; c->rank = rank; c->world = world;
    { std::lock_guard<std::mutex> lk(G->m); G->members.push_back(c); }
    return TSBA_OK;
}
int tsba_comm_stats(void *ctx, int32_t *ranks, int64_t bytes[3]) {
    Ctx *c = (Ctx *)ctx; if (!c) return TSBA_ERR_ARG;
    if (ranks) { int n = c->lgroup ? c->lgroup->world : 1;
        if (c->comm && c->p_count && c->p_count(c->comm, &n) != ncclSuccess) return TSBA_ERR_COMM;
        *ranks = n; }
    if (bytes) { bytes[0] = (int64_t)c->x_trial; bytes[1] = (int64_t)c->x_lin; bytes[2] = (int64_t)c->x_pass; }
    return TSBA_OK;
}
int tsba_debug_set(void *ctx, const tsba_debug_options *d) {
    Ctx *c = (Ctx *)ctx; if (!c) return TSBA_ERR_ARG;
    if (d) c->dbg = *d; else memset(&c->dbg, 0, sizeof(c->dbg));
    return TSBA_OK;
}
int tsba_comm_init(void *ctx, const void *id128, int rank, int world) {
    Ctx *c = (Ctx *)ctx; if (!c || world < 1 || rank < 0 || rank >= world) return TSBA_ERR_ARG;
    hipSetDevice(c->device);
    lgroup_forget(c);                              // (an RCCL communicator replaces an in-process group)
    if (!id128) { c->force_multi = world >= 1; c->rank = 0; c->world = 1; return TSBA_OK; }   // test hook: split kernels, no communicator
    int rc = load_rccl(c); if (rc) return rc;
    ncclUniqueId id; memcpy(&id, id128, 128);
    ncclResult_t r = c->p_init(&c->comm, world, id, rank);
    if (r != ncclSuccess) { set_err(c, std::string("ncclCommInitRank: ") + c->p_errstr(r)); return TSBA_ERR_COMM; }
    c->rank = rank; c->world = world;
    free_problem(c);                               // any resident problem was sharded for the old world size
    return TSBA_OK;
}

} // extern "C"
