// muahuff.hip -- C ABI (include/muahuff.h) over the gfx950 kernels in mh_kernels.hpp.
// Host side: the ABI's NULL checks, HIP calls and kernel launches.  What decides WHAT the device does is computed in
// host-only headers (mh_planner.hpp, mh_sweep_planner.hpp, mh_plan_arena.hpp, mh_select.hpp, mh_worklist.hpp,
// mh_launch.hpp) and so is the walk over stored streams (mh_validate.hpp).
// There is no CPU fallback anywhere in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "mh_abi.hpp"
#include "mh_analysis.hpp"
#include "mh_codec2.hpp"
#include "mh_launch.hpp"
#include "mh_layout.hpp"
#include "mh_packed_measure.hpp"
#include "mh_plan_arena.hpp"
#include "mh_planner.hpp"
#include "mh_range.hpp"
#include "mh_rebin_decode.hpp"
#include "mh_select.hpp"
#include "mh_sweep_planner.hpp"
#include "mh_validate.hpp"
#include "mh_worklist.hpp"
// The library is built with -fvisibility=hidden: the C ABI of include/muahuff.h is ALL it exports
// (tests/test_host.py compares the dynamic symbol table with the header's prototypes).
#pragma GCC visibility push(default)
#include "muahuff.h"
#pragma GCC visibility pop

namespace {

#define MH_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(MH_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),  \
                        __FILE__, __LINE__);                                                 \
    } while (0)

static_assert(mh::kArenaHistSlots == mh::kHistStride && mh::kArenaLutEntries == mh::kLut && sizeof(uint2) == 8 &&
                  mh::kArenaScanBlock == mh::kScanBlock,
              "mh_plan_arena.hpp sizes the scratch regions by the kernels' constants");
static_assert(mh::kGeoRebinTileBytes == mh::kRebinTileBytes && mh::kGeoTr2T == mh::kTr2T && mh::kGeoTr2C == mh::kTr2C &&
                  mh::kGeoScanBlock == mh::kScanBlock && mh::kGeoCompactSegs == mh::kCompactSegs,
              "mh_launch.hpp sizes the grids by the kernels' constants");

// The one device allocation of a plan or a sweep handle, laid out by mh_plan_arena.hpp: the tables part uploaded in
// one copy, the scratch part behind it zeroed.  Synchronises.  Freed with the handle, a half-created one included.
struct DeviceArena {
    uint8_t *base = nullptr;

    DeviceArena() = default;
    DeviceArena(const DeviceArena &) = delete;
    DeviceArena &operator=(const DeviceArena &) = delete;
    ~DeviceArena() { (void)hipFree(base); }
    int create(const mh::Arena &a)
    {
        MH_HIP(hipMalloc(reinterpret_cast<void **>(&base), a.bytes()));
        MH_HIP(hipMemcpy(base, a.tables.get(), a.tables_bytes, hipMemcpyHostToDevice));
        MH_HIP(hipMemset(base + a.tables_bytes, 0, a.scratch_bytes));
        MH_HIP(hipStreamSynchronize(nullptr));
        return MH_OK;
    }
    // the typed view of a region (null where the layout leaves it out)
    template <class T>
    void view(T *&d, const mh::Region &r) const
    {
        d = r.present ? reinterpret_cast<T *>(base + r.off) : nullptr;
    }
};

}  // namespace

// The work list of the last mh_decode_range / mh_decode_rebin call on a plan (mh_worklist.hpp): the same query again
// reuses it as it is on the device.  w keeps the host copy alive until the next call has synchronised.
struct ListCache {
    std::vector<uint32_t> sel;  // the query the list answers; empty: no valid list
    uint64_t t0 = 0, t1 = 0, pitch = 0;
    uint32_t r = 0;  // (0: the range call)
    mh::WorkList w;
    uint8_t *d_list = nullptr, *d_aux = nullptr;  // w.blob; the list's w.naux scratch slots / side words
    size_t cap = 0, aux_cap = 0;

    ListCache() = default;
    ListCache(const ListCache &) = delete;
    ListCache &operator=(const ListCache &) = delete;
    ~ListCache() { (void)hipFree(d_list), (void)hipFree(d_aux); }
    bool same_query(const uint32_t *s, uint32_t n, uint64_t a, uint64_t b, uint32_t r_, uint64_t pitch_) const
    {
        return t0 == a && t1 == b && r == r_ && pitch == pitch_ && sel.size() == n && std::equal(s, s + n, sel.begin());
    }
    const uint8_t *wgs() const { return d_list + w.b_task; }
    const uint8_t *fixes() const { return wgs() + w.b_wg; }
    const uint8_t *fills() const { return fixes() + w.b_fix; }
};

// A codec kernel instance and its dynamic-LDS request, resolved at plan creation (resolve_kernels): the entry points
// launch what the plan holds: mh_encode / mh_decode issue nothing but stream work and stay capturable into a hipGraph.
struct Kernel {
    const void *fn = nullptr;
    size_t lds = 0;
};

struct mh_plan {
    int device = 0;
    mh::PlanHost h;  // everything the planner computed (host copies)
    DeviceArena arena;  // ALL the plan owns on the device but the two work lists; the d_* below are views into it (plan_upload)
    // device tables
    uint64_t *d_ch_off = nullptr, *d_ch_len = nullptr, *d_w0 = nullptr, *d_w1 = nullptr;
    uint8_t *d_skip = nullptr, *d_sclv = nullptr;
    uint32_t *d_sclv16 = nullptr;  // the K rows padded to 16 bytes: one vector load per lane in the in-wave calibration
    uint32_t *d_tile_cnt = nullptr, *d_tile_done = nullptr;  // fused measure: tiles per channel, arrival tickets
    uint32_t *d_codes = nullptr;
    uint32_t *d_seg_ch = nullptr;
    uint64_t *d_seg_first = nullptr, *d_seg_n = nullptr, *d_seg_off = nullptr;
    uint32_t *d_tile_ch = nullptr, *d_tile_n = nullptr;
    uint64_t *d_tile_start = nullptr;
    // device scratch
    unsigned long long *d_hist = nullptr;
    uint8_t *d_peak = nullptr, *d_enc = nullptr;
    uint2 *d_lut = nullptr;
    // shared-table kernels: workgroup tasks (first segment, count); per-wave-table kernels: the
    // segment of every wave task
    mh::WgTask *d_wg_tasks = nullptr;
    mh::WaveTask *d_wave_tasks = nullptr;
    uint64_t *d_scan = nullptr;  // block sums of mh_compact's segment scan
    // calibration windows above kCalDirect samples: tiles for the window-histogram kernel
    uint32_t *d_cal_tile_ch = nullptr, *d_cal_tile_n = nullptr;
    uint64_t *d_cal_tile_start = nullptr;
    unsigned long long *d_calhist = nullptr;
    size_t packed_cal_tiles = 0;  // packed plans: calibration tiles on the device (every window: the pieces are never scanned by k_calibrate)
    unsigned long long *d_acc = nullptr;  // wave-task encoder: per-channel {bits << 24 | finished records} (zero between launches)
    uint32_t *d_err = nullptr;  // decode status word (mh_decode_status): non-zero once a decode abandoned a segment
    Kernel k_enc, k_dec, k_dec_packed, k_range, k_rebin_sat, k_rebin_wide;  // what the entry points launch (resolve_kernels)
    ListCache range, rebin;  // mh_decode_range (scratch slots of cut chunks) / mh_decode_rebin (side words of shared bins)
};

struct mh_sweep {
    int device = 0;
    uint32_t ni = 0;
    std::vector<uint64_t> bounds;  // C * (ni + 1), sorted per channel (mh_sweep_planner.hpp)
    uint64_t n_tiles = 0, n_slots = 0;
    // views into the arena
    uint64_t *d_ch_off = nullptr, *d_tile_start = nullptr, *d_slot_len = nullptr;
    uint32_t *d_tile_ch = nullptr, *d_tile_n = nullptr, *d_tile_slot = nullptr;
    unsigned long long *d_scratch = nullptr;
    DeviceArena arena;  // what the d_* above point into
};

// device operations run on the plan's device: its tables live there
static int check_device(int device, const char *who)
{
    int d = -1;
    MH_HIP(hipGetDevice(&d));
    if (d != device)
        return fail(MH_ERR_ARG, "%s: the plan was created on device %d, the current device is %d", who, device, d);
    return MH_OK;
}

static mh::CalArgs calibrate_args(const mh_plan *p, const uint8_t *data, uint64_t *cutoff, uint32_t *cal_hist,
                                  uint8_t *peak, uint8_t *enc, unsigned long long *zero_hist,
                                  unsigned long long *zero_bits, uint8_t *skip_dst)
{
    const mh_plan_info_t &I = p->h.info;
    mh::CalArgs a;
    a.zero_hist = zero_hist;
    a.zero_bits = zero_bits;
    a.skip_src = p->d_skip;
    a.skip_dst = skip_dst;
    a.data = data;
    a.ch_off = p->d_ch_off;
    a.ch_len = p->d_ch_len;
    a.sclv = p->d_sclv;
    a.sclv16 = p->d_sclv16;
    a.codes = p->d_codes;
    a.C = I.C;
    a.S = I.S;
    a.h = I.h;
    a.mode = I.mode;
    a.K = I.K;
    a.cutoff = cutoff;
    a.cal_sorted = cal_hist;
    a.peak = peak;
    a.enc = enc;
    a.lut = p->d_lut;
    a.pre_hist = nullptr;
    return a;
}

static mh::HistArgs hist_args(const uint8_t *data, const uint64_t *ch_off, const uint32_t *tile_ch, const uint64_t *tile_start,
                              const uint32_t *tile_n, unsigned long long *hist, const uint32_t *tile_slot)
{
    mh::HistArgs a{};
    a.data = data;
    a.ch_off = ch_off;
    a.tile_ch = tile_ch;
    a.tile_start = tile_start;
    a.tile_n = tile_n;
    a.hist = hist;
    a.tile_slot = tile_slot;
    return a;
}

static int launch_calibrate(mh_plan *p, const uint8_t *data, uint64_t *cutoff, uint32_t *cal_hist,
                            uint8_t *peak, uint8_t *enc, hipStream_t st, unsigned long long *zero_hist,
                            unsigned long long *zero_bits, uint8_t *skip_dst)
{
    const mh_plan_info_t &I = p->h.info;
    mh::CalArgs a = calibrate_args(p, data, cutoff, cal_hist, peak, enc, zero_hist, zero_bits, skip_dst);
    if (!p->h.cal_tile_ch.empty()) {  // long calibration windows (2^h > kCalDirect): tiled histogram first
        MH_HIP(hipMemsetAsync(p->d_calhist, 0, (size_t)a.C * mh::kHistStride * sizeof(unsigned long long), st));
        const mh::HistArgs ha = hist_args(data, p->d_ch_off, p->d_cal_tile_ch, p->d_cal_tile_start, p->d_cal_tile_n, p->d_calhist, nullptr);
        hipLaunchKernelGGL(mh::k_hist2<4>, dim3((unsigned)p->h.cal_tile_ch.size()), dim3(256), 0, st, ha, I.S);
        a.pre_hist = p->d_calhist;
    }
    hipLaunchKernelGGL(mh::k_calibrate, dim3((a.C + 3) / 4), dim3(256), 0, st, a);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

// window or calibration histogram of a packed plan over `nt` of its tiles (mh_packed_measure.hpp)
static void launch_hist_packed(const mh_plan *p, const uint8_t *data, const uint32_t *tile_ch, const uint64_t *tile_start,
                               const uint32_t *tile_n, unsigned long long *hist, size_t nt, hipStream_t st)
{
    mh::PackedHistArgs a;
    a.data = data;
    a.ch_off = p->d_ch_off;
    a.tile_ch = tile_ch;
    a.tile_start = tile_start;
    a.tile_n = tile_n;
    a.hist = hist;
    a.stride = p->h.chunk_stride ? p->h.chunk_stride : (uint64_t)MH_CHUNK * p->h.input_bits / 8;
    a.S = p->h.info.S;
    const dim3 g((unsigned)nt), b(256);
    if (p->h.input_bits == 2) {
        hipLaunchKernelGGL((mh::k_hist_packed<2, 3>), g, b, 0, st, a);
        return;
    }
    switch (a.S) {
    case 2: hipLaunchKernelGGL((mh::k_hist_packed<4, 1>), g, b, 0, st, a); break;
    case 3: hipLaunchKernelGGL((mh::k_hist_packed<4, 2>), g, b, 0, st, a); break;
    case 4: hipLaunchKernelGGL((mh::k_hist_packed<4, 3>), g, b, 0, st, a); break;
    case 5: hipLaunchKernelGGL((mh::k_hist_packed<4, 4>), g, b, 0, st, a); break;
    case 6: hipLaunchKernelGGL((mh::k_hist_packed<4, 5>), g, b, 0, st, a); break;
    case 7: hipLaunchKernelGGL((mh::k_hist_packed<4, 6>), g, b, 0, st, a); break;
    case 8: hipLaunchKernelGGL((mh::k_hist_packed<4, 7>), g, b, 0, st, a); break;
    case 9: hipLaunchKernelGGL((mh::k_hist_packed<4, 8>), g, b, 0, st, a); break;
    default: hipLaunchKernelGGL((mh::k_hist_packed<4, 9>), g, b, 0, st, a); break;
    }
}

template <int NS>
static void launch_hist(const mh::HistArgs &a, uint64_t n_tiles, hipStream_t st)
{
    hipLaunchKernelGGL(mh::k_hist<NS>, dim3((unsigned)n_tiles), dim3(256), 0, st, a);
}

static int launch(const Kernel &k, uint32_t grid, const void *args, hipStream_t st)
{
    void *argv[] = {const_cast<void *>(args)};
    MH_HIP(hipLaunchKernel(k.fn, dim3(grid), dim3(256), argv, k.lds, st));
    return MH_OK;
}

static int prepare_kernel(const void *kern, size_t lds, bool needs_lds_base_0)
{
    if (needs_lds_base_0) {
        hipFuncAttributes fa;
        MH_HIP(hipFuncGetAttributes(&fa, kern));
        if (fa.sharedSizeBytes != 0)
            return fail(MH_ERR_HIP, "decode kernel has %zu bytes of static LDS: its table would not sit at LDS offset 0",
                        (size_t)fa.sharedSizeBytes);
    }
    if (lds > 64 * 1024)
        MH_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MH_OK;
}

// f(std::integral_constant<size_t, i>) for every i < N in turn: the entries of a selection table as constant expressions.
// The instances a visitor names are compiled in its order, which is their order in the code object.
template <class F, size_t... I>
static void for_each_index(F f, std::index_sequence<I...>) { (..., f(std::integral_constant<size_t, I>{})); }

// THE place an encoder pick becomes its template instance ...
static const void *encoder_instance(const mh::EncPick &p)
{
    const void *k = nullptr;
    for_each_index([&](auto i) {
        constexpr mh::EncPick E = mh::kEncInsts[decltype(i)::value];
        if (E.LC == p.LC && E.PB == p.PB && E.PK == p.PK)
            k = p.wave ? (const void *)mh::k_encode2w<E.LC, E.PB, E.PK> : (const void *)mh::k_encode2<E.LC, E.PB, E.PK>;
    }, std::make_index_sequence<sizeof(mh::kEncInsts) / sizeof(mh::kEncInsts[0])>{});
    return k;
}

// ... and a decoder pick its (nullptr: not built, mh::dec_built)
template <size_t I, mh::DecForm F, uint32_t PO>
static const void *decoder_instance()
{
    constexpr mh::DecRung R = mh::kDecRungs[I];
    if constexpr (!mh::dec_built(I, F, PO)) return nullptr;
    else if constexpr (F == mh::kDecode2w) return (const void *)mh::k_decode2w<R.K, R.M, R.NR, R.RL, R.HY, R.DUAL, PO>;
    else if constexpr (F == mh::kDecode2) return (const void *)mh::k_decode2<R.K, R.M, R.NR, R.RL, R.HY, PO>;
    else if constexpr (F == mh::kDecodeRange) return (const void *)mh::k_decode_range<R.K, R.M, R.NR, R.RL, R.HY>;
    else return (const void *)mh::k_decode_rebin<R.K, R.M, R.NR, R.RL, R.HY, F == mh::kDecodeRebinSat>;
}

static const void *decoder_instance(const mh::DecPick &p)
{
    struct Group { mh::DecForm a, b; uint32_t po; };  // two forms side by side per rung; all rungs of a group before the next
    static constexpr Group G[] = {{mh::kDecodeRange, mh::kDecodeRange, 0}, {mh::kDecodeRebinSat, mh::kDecodeRebinWide, 0},
                                  {mh::kDecode2w, mh::kDecode2, 2}, {mh::kDecode2w, mh::kDecode2, 4}, {mh::kDecode2w, mh::kDecode2, 0}};
    const void *k = nullptr;
    for_each_index([&](auto i) {
        constexpr Group g = G[decltype(i)::value / mh::kDecRungCount];
        constexpr size_t I = decltype(i)::value % mh::kDecRungCount;
        const void *a = decoder_instance<I, g.a, g.po>(), *b = decoder_instance<I, g.b, g.po>();
        if (I == p.rung && g.po == p.po && (p.form == g.a || p.form == g.b)) k = p.form == g.a ? a : b;
    }, std::make_index_sequence<5 * mh::kDecRungCount>{});
    return k;
}

// The kernel of a pick and its LDS request, prepared: the dynamic-LDS limit raised where the request needs it, and no
// static LDS in the kernels that address their table by raw LDS offset (k_decode2 with K = 2, range, re-bin).
static int resolve(Kernel *k, const void *fn, size_t lds, bool needs_lds_base_0)
{
    if (!fn) return fail(MH_ERR_ARG, "mh_plan_create: no kernel instance is built for this plan");
    *k = Kernel{fn, lds};
    return prepare_kernel(fn, lds, needs_lds_base_0);
}

static int resolve(Kernel *k, const mh::DecPick &p, uint32_t W)
{
    const bool base0 = p.form != mh::kDecode2w && (p.form != mh::kDecode2 || mh::kDecRungs[p.rung].K == 2);
    return resolve(k, decoder_instance(p), mh::dec_lds_bytes(p, W), base0);
}

static mh::TaskArgs task_args(const mh_plan *p)
{
    mh::TaskArgs t{};
    if (p->h.use_wave_tasks) {  // one wave per segment, longest first
        t.wt = p->d_wave_tasks;
        t.ntask = (uint32_t)p->h.wave_tasks.size();
    } else {                    // one workgroup per <= 4 consecutive segments of a channel
        t.wg = p->d_wg_tasks;
        t.ntask = (uint32_t)p->h.wg_tasks.size();
        t.seg_samples = p->h.info.seg_chunks * MH_CHUNK;
        t.seg_src_stride = p->h.seg_src_stride;
        t.slot_full = p->h.slot_full;
    }
    return t;
}

// launch of a codec kernel (a: Enc2Args, Dec2Args) in the plan's task form: a workgroup per workgroup task or per four wave tasks
template <class A>
static int launch_tasks(const mh_plan *p, const Kernel &k, const A &a, hipStream_t st)
{
    return launch(k, p->h.use_wave_tasks ? (a.t.ntask + 3) / 4 : a.t.ntask, &a, st);
}

// the kernels this plan will launch (once, at plan creation)
static int resolve_kernels(mh_plan *p)
{
    const mh::PlanHost &H = p->h;
    const uint32_t L = H.info.maxlen, W = H.W;
    const mh::EncPick e = mh::enc_pick(L, H.info.S, H.input_bits, H.use_wave_tasks);
    int rc = resolve(&p->k_enc, encoder_instance(e), mh::enc_lds_bytes(e, L, task_args(p).ntask), false);
    if (rc || (rc = resolve(&p->k_dec, mh::dec_pick(L, W, H.use_wave_tasks, 0), W))) return rc;
    if (H.input_bits == mh::packed_out_bits(H.info.S))  // a plan mh_decode_packed accepts
        return resolve(&p->k_dec_packed, mh::dec_pick(L, W, H.use_wave_tasks, H.input_bits), W);
    if (H.input_bits != 8) return MH_OK;
    const mh::DecRungId r = mh::dec_pick(L, W, false, 0).rung;  // a plan mh_decode_range / mh_decode_rebin accept
    if ((rc = resolve(&p->k_range, {r, mh::kDecodeRange, 0}, W)) || (rc = resolve(&p->k_rebin_sat, {r, mh::kDecodeRebinSat, 0}, W)))
        return rc;
    return resolve(&p->k_rebin_wide, {r, mh::kDecodeRebinWide, 0}, W);
}

#pragma GCC visibility push(default)
extern "C" {

int mh_version(void) { return MH_VERSION; }

const char *mh_last_error(void) { return g_err; }

int mh_device_info(int device, int *cu_count, uint64_t *hbm_bytes, char *name, int name_cap,
                   char *arch, int arch_cap)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(MH_ERR_NO_DEVICE, "no HIP device visible (libmuahuff has no CPU fallback)");
    if (device < 0 || device >= n) return fail(MH_ERR_ARG, "device %d out of range (%d)", device, n);
    hipDeviceProp_t p;
    MH_HIP(hipGetDeviceProperties(&p, device));
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (uint64_t)p.totalGlobalMem;
    if (name && name_cap > 0) snprintf(name, (size_t)name_cap, "%s", p.name);
    if (arch && arch_cap > 0) snprintf(arch, (size_t)arch_cap, "%s", p.gcnArchName);
    return MH_OK;
}

int mh_codebook(const uint8_t *sclv_row, int S, uint16_t *code, uint8_t *len)
{
    if (!sclv_row || !code || !len || S < 2 || S > MH_LUT_SYMS) return fail(MH_ERR_ARG, "mh_codebook: bad argument");
    uint32_t m;
    if (mh::check_sclv_row(sclv_row, S, &m) != MH_OK)
        return fail(MH_ERR_SCLV, "SCLV row is not a non-decreasing complete prefix-code length vector");
    mh::canonical_codes(sclv_row, S, code, len);
    return MH_OK;
}

int mh_approx_sort_perm(int S, int peak, uint8_t *idx)
{
    if (!idx || S < 2 || S > MH_LUT_SYMS || peak < 0 || peak >= S)
        return fail(MH_ERR_ARG, "mh_approx_sort_perm: bad argument");
    for (int k = 0; k < S; ++k) idx[k] = (uint8_t)mh::symbol_of_rank(MH_MODE_APPROX, S, peak, k);
    return MH_OK;
}

int mh_plan_destroy(mh_plan *p)
{
    delete p;  // (the arena and the work-list caches free what they hold)
    return MH_OK;
}

// device side of plan creation: the arena (mh_plan_arena.hpp) and the views into it
static int plan_upload(mh_plan *p)
{
    const mh::PlanArena a = mh::plan_arena(p->h);
    if (int rc = p->arena.create(a)) return rc;
    const DeviceArena &d = p->arena;
    d.view(p->d_sclv16, a.sclv16), d.view(p->d_tile_cnt, a.tile_cnt), d.view(p->d_ch_off, a.ch_off), d.view(p->d_ch_len, a.ch_len);
    d.view(p->d_w0, a.w0), d.view(p->d_w1, a.w1), d.view(p->d_skip, a.skip), d.view(p->d_sclv, a.sclv), d.view(p->d_codes, a.codes);
    d.view(p->d_seg_ch, a.seg_ch), d.view(p->d_seg_first, a.seg_first), d.view(p->d_seg_n, a.seg_n), d.view(p->d_seg_off, a.seg_off);
    d.view(p->d_tile_ch, a.tile_ch), d.view(p->d_tile_n, a.tile_n), d.view(p->d_tile_start, a.tile_start);
    d.view(p->d_wg_tasks, a.wg_tasks), d.view(p->d_wave_tasks, a.wave_tasks);
    d.view(p->d_cal_tile_ch, a.cal_tile_ch), d.view(p->d_cal_tile_n, a.cal_tile_n), d.view(p->d_cal_tile_start, a.cal_tile_start);
    d.view(p->d_tile_done, a.tile_done), d.view(p->d_hist, a.hist), d.view(p->d_peak, a.peak), d.view(p->d_enc, a.enc);
    d.view(p->d_lut, a.lut), d.view(p->d_scan, a.scan), d.view(p->d_err, a.err), d.view(p->d_acc, a.acc), d.view(p->d_calhist, a.calhist);
    if (p->h.input_bits != 8) p->packed_cal_tiles = a.n_cal_tiles;
    return MH_OK;
}

// the first n entries of the directory, into those of the four arrays the caller asked for
static void copy_segments(const mh::PlanHost &H, size_t n, uint32_t *seg_ch, uint64_t *seg_first, uint64_t *seg_n, uint64_t *seg_off)
{
    if (seg_ch && n) memcpy(seg_ch, H.seg_ch.data(), n * sizeof(uint32_t));
    if (seg_first && n) memcpy(seg_first, H.seg_first.data(), n * sizeof(uint64_t));
    if (seg_n && n) memcpy(seg_n, H.seg_n.data(), n * sizeof(uint64_t));
    if (seg_off && n) memcpy(seg_off, H.seg_off.data(), n * sizeof(uint64_t));
}

int mh_plan_query(const uint64_t *ch_len, uint32_t C, uint32_t S, uint32_t h, uint32_t mode, uint32_t window,
                  const uint8_t *sclv, uint32_t K, uint32_t seg_chunks, mh_plan_info_t *info, uint32_t *seg_ch,
                  uint64_t *seg_first, uint64_t *seg_n, uint64_t *seg_off, uint64_t seg_cap)
{
    if (!ch_len || !sclv || !info) return fail(MH_ERR_ARG, "mh_plan_query: NULL argument");
    mh::PlanHost H;
    mh::Msg m;
    if (int rc = mh::plan_host_of_args(m, ch_len, C, S, h, mode, window, sclv, K, seg_chunks, H)) return fail(rc, m);
    *info = H.info;
    copy_segments(H, H.seg_ch.size() < seg_cap ? H.seg_ch.size() : (size_t)seg_cap, seg_ch, seg_first, seg_n, seg_off);
    return MH_OK;
}

int mh_plan_create(mh_plan **plan, const uint64_t *ch_off, const uint64_t *ch_len, uint32_t C,
                   uint32_t S, uint32_t h, uint32_t mode, uint32_t window, const uint8_t *sclv,
                   uint32_t K, uint32_t seg_chunks)
{
    return mh_plan_create_packed(plan, ch_off, ch_len, C, S, h, mode, window, sclv, K, seg_chunks, 8, 0);
}

int mh_plan_create_packed(mh_plan **plan, const uint64_t *ch_off, const uint64_t *ch_len, uint32_t C,
                          uint32_t S, uint32_t h, uint32_t mode, uint32_t window, const uint8_t *sclv,
                          uint32_t K, uint32_t seg_chunks, uint32_t input_bits, uint64_t chunk_stride)
{
    if (!plan || !ch_off || !ch_len || !sclv) return fail(MH_ERR_ARG, "mh_plan_create: NULL argument");
    *plan = nullptr;
    if (input_bits != 8 && input_bits != 4 && input_bits != 2)
        return fail(MH_ERR_ARG, "input_bits=%u (8, 4 or 2)", input_bits);
    if (input_bits != 8 && (window & ~MH_WIN_REV2_SEGMENTS) != MH_WIN_FULL)
        return fail(MH_ERR_ARG, "packed input needs the whole-channel window (MH_WIN_FULL)");
    if (input_bits == 2 && S > 4) return fail(MH_ERR_ARG, "2-bit input holds symbols 0..3: S=%u is above 4", S);
    if (!mh::chunk_stride_ok(chunk_stride, input_bits))
        return fail(MH_ERR_ARG, "chunk_stride=%llu: packed input only, a multiple of 16, at least one chunk",
                    (unsigned long long)chunk_stride);
    mh_plan_info_t I;
    mh::Msg m;
    if (int rc = mh::plan_args(m, ch_len, C, S, h, mode, window, sclv, K, seg_chunks, &I)) return fail(rc, m);
    int ndev = 0, dev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(MH_ERR_NO_DEVICE, "no HIP device visible (libmuahuff has no CPU fallback)");
    MH_HIP(hipGetDevice(&dev));
    mh_plan *p = new (std::nothrow) mh_plan;
    if (!p) return fail(MH_ERR_ARG, "out of host memory");
    p->device = dev;
    p->h.info = I;
    p->h.input_bits = input_bits;
    p->h.chunk_stride = chunk_stride;
    mh::plan_host_build(p->h, ch_off, ch_len, sclv);
    if (p->h.seg_ch.size() > 0xFFFFFFF0ull) {  // segment and task indices are 32-bit on the device
        const size_t nseg = p->h.seg_ch.size();
        mh_plan_destroy(p);
        return fail(MH_ERR_ARG, "mh_plan_create: %zu segments exceed the 32-bit directory", nseg);
    }
    int rc = plan_upload(p);
    if (rc == MH_OK) rc = resolve_kernels(p);
    if (rc != MH_OK) {
        mh_plan_destroy(p);
        return rc;
    }
    *plan = p;
    return MH_OK;
}

int mh_plan_info(const mh_plan *plan, mh_plan_info_t *info)
{
    if (!plan || !info) return fail(MH_ERR_ARG, "mh_plan_info: NULL argument");
    *info = plan->h.info;
    return MH_OK;
}

int mh_plan_segments(const mh_plan *plan, uint32_t *seg_ch, uint64_t *seg_first, uint64_t *seg_n,
                     uint64_t *seg_off)
{
    if (!plan) return fail(MH_ERR_ARG, "mh_plan_segments: NULL plan");
    copy_segments(plan->h, plan->h.seg_ch.size(), seg_ch, seg_first, seg_n, seg_off);
    return MH_OK;
}

int mh_measure(mh_plan *p, const uint8_t *data, uint64_t *cutoff, uint32_t *cal_hist,
               uint8_t *peak, uint8_t *enc, uint64_t *post_hist, uint64_t *bits,
               uint8_t *skipped, void *stream)
{
    if (!p || !data) return fail(MH_ERR_ARG, "mh_measure: NULL argument");
    if (int rc_ = check_device(p->device, "mh_measure")) return rc_;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *pk = peak ? peak : p->d_peak, *en = enc ? enc : p->d_enc;
    mh::FinArgs f;
    f.hist = p->d_hist;
    f.w0 = p->d_w0;
    f.w1 = p->d_w1;
    f.skipflag = p->d_skip;
    f.peak = pk;
    f.enc = en;
    f.sclv = p->d_sclv;
    f.sclv16 = p->d_sclv16;
    f.C = p->h.info.C;
    f.S = p->h.info.S;
    f.mode = p->h.info.mode;
    f.post = post_hist;
    f.bits = bits;
    f.skipped = skipped;
    // Launch-bound shapes (mh_planner.hpp: kFusedMeasureChannels): ONE launch.
    // The workgroup that adds a channel's last tile to the histogram calibrates and prices the channel
    // (measure_tail); the histogram scratch and the tickets are left zero for the next call.
    if (p->h.input_bits != 8) {
        // Packed pieces: the tiled bit-count kernel histograms the calibration windows, k_calibrate turns those counts
        // into (peak, encoder) -- it never looks at the pieces -- and clears the window histogram, which the same
        // kernel then fills over the planner's window tiles.  Never the one-launch form: its tail calibrates by scanning
        // bytes.  Five enqueues on `stream`, nothing else.
        MH_HIP(hipMemsetAsync(p->d_calhist, 0, (size_t)f.C * mh::kHistStride * sizeof(unsigned long long), st));
        launch_hist_packed(p, data, p->d_cal_tile_ch, p->d_cal_tile_start, p->d_cal_tile_n, p->d_calhist, p->packed_cal_tiles, st);
        mh::CalArgs a = calibrate_args(p, data, cutoff, cal_hist, pk, en, p->d_hist, nullptr, nullptr);
        a.pre_hist = p->d_calhist;
        hipLaunchKernelGGL(mh::k_calibrate, dim3((a.C + 3) / 4), dim3(256), 0, st, a);
        launch_hist_packed(p, data, p->d_tile_ch, p->d_tile_start, p->d_tile_n, p->d_hist, p->h.tile_ch.size(), st);
        hipLaunchKernelGGL(mh::k_finalize, dim3((f.C + 255) / 256), dim3(256), 0, st, f);
        MH_HIP(hipGetLastError());
        return MH_OK;
    }
    const bool fused = p->h.measure_fused;
    if (!fused) {
        int rc = launch_calibrate(p, data, cutoff, cal_hist, pk, en, st, p->d_hist, nullptr, nullptr);
        if (rc) return rc;
    }
    if (!p->h.tile_ch.empty()) {
        mh::HistArgs a = hist_args(data, p->d_ch_off, p->d_tile_ch, p->d_tile_start, p->d_tile_n, p->d_hist, nullptr);
        if (fused) {
            a.tile_cnt = p->d_tile_cnt;
            a.tile_done = p->d_tile_done;
            a.cal = calibrate_args(p, data, cutoff, cal_hist, pk, en, nullptr, nullptr, nullptr);
            a.fin = f;
        }
        const uint64_t n_tiles = p->h.tile_ch.size();
        const unsigned nt = (unsigned)n_tiles;
        if (p->h.info.S == 2)
            launch_hist<1>(a, n_tiles, st);  // byte-compare kernel: already at the read floor
        else if (p->h.info.S == 3)
            launch_hist<2>(a, n_tiles, st);
        else if (p->h.info.S <= 8)  // pair-LUT histogram, 3-bit pair packing
            hipLaunchKernelGGL(mh::k_hist2<3>, dim3(nt), dim3(256), 0, st, a, p->h.info.S);
        else                      // S = 9, 10: 4-bit packing, xor-swizzled
            hipLaunchKernelGGL(mh::k_hist2<4>, dim3(nt), dim3(256), 0, st, a, p->h.info.S);
        MH_HIP(hipGetLastError());
    }
    if (fused) return MH_OK;
    hipLaunchKernelGGL(mh::k_finalize, dim3((f.C + 255) / 256), dim3(256), 0, st, f);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

static int check_payload_cap(const mh_plan *p, uint64_t payload_cap_words)
{
    if (payload_cap_words < p->h.info.payload_cap_words)
        return fail(MH_ERR_CAPACITY, "payload buffer holds %llu words, plan needs %llu",
                    (unsigned long long)payload_cap_words,
                    (unsigned long long)p->h.info.payload_cap_words);
    return MH_OK;
}

// cal_mode: see EncArgs.  Modes 1 and 2 exist for wave-task plans only.
static int encode_common(mh_plan *p, const uint8_t *data, uint32_t *payload, uint64_t *seg_words,
                         uint64_t *ch_bits, uint32_t cal_mode, const uint8_t *peak_in, const uint8_t *enc_in,
                         uint8_t *peak_out, uint8_t *enc_out, uint8_t *skip_out, hipStream_t st)
{
    if (cal_mode == 0 && p->h.info.n_segments == 0) return MH_OK;
    mh::EncArgs a;
    a.cal_mode = cal_mode;
    a.chunk_stride = p->h.chunk_stride;
    a.S = p->h.info.S;
    a.mode = p->h.info.mode;
    a.K = p->h.info.K;
    a.sclv = p->d_sclv;
    a.sclv16 = p->d_sclv16;
    a.codes = p->d_codes;
    a.peak_in = peak_in;
    a.enc_in = enc_in;
    a.peak_out = peak_out;
    a.enc_out = enc_out;
    a.skip_out = skip_out;
    a.acc = p->d_acc;
    a.data = data;
    a.ch_off = p->d_ch_off;
    a.w0 = p->d_w0;
    a.seg_ch = p->d_seg_ch;
    a.seg_first = p->d_seg_first;
    a.seg_n = p->d_seg_n;
    a.seg_off = p->d_seg_off;
    a.lut = p->d_lut;
    a.payload = payload;
    a.seg_words = seg_words;
    a.ch_bits = reinterpret_cast<unsigned long long *>(ch_bits);
    a.nseg = (uint32_t)p->h.info.n_segments;
    a.stage_dw = mh::enc_stage_dw(p->h.info.maxlen);
    mh::Enc2Args a2;
    a2.e = a;
    a2.t = task_args(p);
    return launch_tasks(p, p->k_enc, a2, st);
}

int mh_encode(mh_plan *p, const uint8_t *data, uint32_t *payload, uint64_t payload_cap_words,
              uint64_t *seg_words, uint64_t *ch_bits, uint8_t *peak, uint8_t *enc,
              uint8_t *skipped, void *stream)
{
    if (!p || !data || !payload || !seg_words || !ch_bits)
        return fail(MH_ERR_ARG, "mh_encode: NULL argument");
    if (p->h.input_bits != 8) return fail(MH_ERR_ARG, "mh_encode: this plan reads packed pieces (mh_encode_preset only)");
    if (int rc_ = check_device(p->device, "mh_encode")) return rc_;
    if (int rc_ = check_payload_cap(p, payload_cap_words)) return rc_;
    hipStream_t st = (hipStream_t)stream;
    if (p->h.fused_calibration && p->h.tickets_fit)  // short channels: every wave calibrates its own channel, one launch in all
        return encode_common(p, data, payload, seg_words, ch_bits, 1u, nullptr, nullptr, peak, enc, skipped, st);
    uint8_t *pk = peak ? peak : p->d_peak, *en = enc ? enc : p->d_enc;
    int rc = launch_calibrate(p, data, nullptr, nullptr, pk, en, st, nullptr,
                              reinterpret_cast<unsigned long long *>(ch_bits), skipped);
    if (rc) return rc;
    return encode_common(p, data, payload, seg_words, ch_bits, 0u, nullptr, nullptr, nullptr, nullptr, nullptr, st);
}

int mh_encode_preset(mh_plan *p, const uint8_t *data, const uint8_t *peak, const uint8_t *enc,
                     uint32_t *payload, uint64_t payload_cap_words, uint64_t *seg_words,
                     uint64_t *ch_bits, void *stream)
{
    if (!p || !data || !peak || !enc || !payload || !seg_words || !ch_bits)
        return fail(MH_ERR_ARG, "mh_encode_preset: NULL argument");
    if (int rc_ = check_device(p->device, "mh_encode_preset")) return rc_;
    if (int rc_ = check_payload_cap(p, payload_cap_words)) return rc_;
    hipStream_t st = (hipStream_t)stream;
    if (p->h.use_wave_tasks && p->h.tickets_fit)  // the waves build their tables from the preset word themselves: one launch
        return encode_common(p, data, payload, seg_words, ch_bits, 2u, peak, enc, nullptr, nullptr, nullptr, st);
    hipLaunchKernelGGL(mh::k_lut_preset, dim3((p->h.info.C + 15) / 16), dim3(256), 0, st, peak, enc,
                       (const uint32_t *)p->d_codes, p->h.info.C, p->h.info.S, p->h.info.mode, p->h.info.K, p->d_lut,
                       reinterpret_cast<unsigned long long *>(ch_bits), (uint8_t *)nullptr, (uint8_t *)nullptr);
    MH_HIP(hipGetLastError());
    return encode_common(p, data, payload, seg_words, ch_bits, 0u, nullptr, nullptr, nullptr, nullptr, nullptr, st);
}

// arguments of mh_decode / mh_decode_packed: both kernel families build their tables themselves from (peak, enc), one launch
static mh::Dec2Args decode_args(const mh_plan *p, const uint32_t *payload, uint64_t payload_words, const uint64_t *seg_off,
                                const uint8_t *peak, const uint8_t *enc, uint8_t *out)
{
    mh::Dec2Args a;
    a.d.payload = payload;
    a.d.ch_off = p->d_ch_off;
    a.d.w0 = p->d_w0;
    a.d.seg_ch = p->d_seg_ch;
    a.d.seg_first = p->d_seg_first;
    a.d.seg_n = p->d_seg_n;
    a.d.seg_off = seg_off ? seg_off : p->d_seg_off;
    a.d.out = out;
    a.d.nseg = (uint32_t)p->h.info.n_segments;
    a.d.payload_words = payload_words;
    a.d.err = p->d_err;
    a.d.epoch = 1u;  // the status word is a sticky flag (mh_decode_status reads and clears it)
    a.t = task_args(p);
    a.W = p->h.W;
    a.peak = peak;
    a.enc = enc;
    a.codes = p->d_codes;
    a.S = p->h.info.S;
    a.mode = p->h.info.mode;
    a.nK = p->h.info.K;
    a.plan_slots = seg_off ? 0u : 1u;
    a.cstride = p->h.chunk_stride ? p->h.chunk_stride : (uint64_t)(MH_CHUNK / MH_PIECE) * p->h.input_bits * 2;
    return a;
}

int mh_decode(mh_plan *p, const uint32_t *payload, uint64_t payload_words, const uint64_t *seg_off,
              const uint8_t *peak, const uint8_t *enc, uint8_t *out, void *stream)
{
    if (!p || !payload || !peak || !enc || !out) return fail(MH_ERR_ARG, "mh_decode: NULL argument");
    if (p->h.input_bits != 8)  // a packed plan's offsets describe the packed buffer, not a byte layout to decode into
        return fail(MH_ERR_ARG, "mh_decode: this plan reads packed pieces (mh_encode_preset only); decode with a byte-layout plan");
    if (int rc_ = check_device(p->device, "mh_decode")) return rc_;
    if (p->h.info.n_segments == 0) return MH_OK;
    return launch_tasks(p, p->k_dec, decode_args(p, payload, payload_words, seg_off, peak, enc, out), (hipStream_t)stream);
}

int mh_decode_packed(mh_plan *p, const uint32_t *payload, uint64_t payload_words, const uint64_t *seg_off,
                     const uint8_t *peak, const uint8_t *enc, uint8_t *out, void *stream)
{
    if (!p || !payload || !peak || !enc || !out) return fail(MH_ERR_ARG, "mh_decode_packed: NULL argument");
    if (p->h.input_bits == 8)
        return fail(MH_ERR_ARG, "mh_decode_packed: this plan describes a byte layout; decode it with mh_decode");
    if (p->h.input_bits != mh::packed_out_bits(p->h.info.S))
        return fail(MH_ERR_ARG, "mh_decode_packed: S=%u decodes to %u-bit pieces, the plan holds %u-bit ones", p->h.info.S,
                    mh::packed_out_bits(p->h.info.S), p->h.input_bits);
    if (int rc_ = check_device(p->device, "mh_decode_packed")) return rc_;
    if (p->h.info.n_segments == 0) return MH_OK;
    return launch_tasks(p, p->k_dec_packed, decode_args(p, payload, payload_words, seg_off, peak, enc, out), (hipStream_t)stream);
}

int mh_decode_status(mh_plan *p, uint32_t *flags, void *stream)
{
    if (!p || !flags) return fail(MH_ERR_ARG, "mh_decode_status: NULL argument");
    if (int rc_ = check_device(p->device, "mh_decode_status")) return rc_;
    uint32_t seen = 0;
    MH_HIP(hipMemcpyAsync(&seen, p->d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    MH_HIP(hipStreamSynchronize((hipStream_t)stream));
    // sticky: any decode since the last status call that abandoned a segment has raised the word -- direct
    // calls and replays of a captured decode alike (a captured kernel carries no per-call state)
    *flags = seen ? 1u : 0u;
    if (seen) {
        MH_HIP(hipMemsetAsync(p->d_err, 0, sizeof(uint32_t), (hipStream_t)stream));
        MH_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
    return MH_OK;
}

// grow-or-keep of one of a ListCache's device buffers
static int grow(uint8_t **d, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return MH_OK;
    if (*d) MH_HIP(hipFree(*d));
    *d = nullptr;
    *cap = 0;
    MH_HIP(hipMalloc(reinterpret_cast<void **>(d), bytes));
    *cap = bytes;
    return MH_OK;
}

// The list `w` of the query (sel, t0, t1, r, out_pitch) becomes the cache's: uploaded in one copy, with room for its
// w.naux auxiliary slots of aux_unit bytes.  Synchronises `st` first: the previous call's kernels may still read the
// buffers (one stream at a time per plan).  The cache holds no valid list from the first line until the copy is enqueued.
static int upload_list(ListCache &c, mh::WorkList &&w, size_t aux_unit, const uint32_t *sel, uint32_t n_sel, uint64_t t0,
                       uint64_t t1, uint32_t r, uint64_t out_pitch, hipStream_t st)
{
    c.sel.clear();
    MH_HIP(hipStreamSynchronize(st));
    int rc;
    if ((rc = grow(&c.d_list, &c.cap, w.blob.size())) || (rc = grow(&c.d_aux, &c.aux_cap, (size_t)(w.naux ? w.naux : 1) * aux_unit)))
        return rc;
    c.w = std::move(w);
    // (never empty: every row of a non-empty query yields a task or a fill record)
    MH_HIP(hipMemcpyAsync(c.d_list, c.w.blob.data(), c.w.blob.size(), hipMemcpyHostToDevice, st));
    c.sel.assign(sel, sel + n_sel);
    c.t0 = t0;
    c.t1 = t1;
    c.r = r;
    c.pitch = out_pitch;
    return MH_OK;
}

// What mh_decode_range and mh_decode_rebin (`who`) ask of their arguments.  r: the bin factor, 1 for the range call,
// whose rows are then t1 - t0 elements long and whose bin-factor checks cannot fire.  *empty: nothing to decode.
static int check_range_call(const char *who, const mh_plan *p, const uint32_t *payload, const uint64_t *seg_off, const uint32_t *sel,
                            uint32_t n_sel, uint64_t t0, uint64_t t1, uint32_t r, const uint8_t *peak, const uint8_t *enc,
                            const void *out, uint64_t out_pitch, bool *empty)
{
    if (!p || (n_sel && !sel)) return fail(MH_ERR_ARG, "%s: NULL argument", who);
    if (p->h.input_bits != 8)
        return fail(MH_ERR_ARG, "%s: this plan reads packed pieces (mh_encode_preset only); decode with a byte-layout plan", who);
    if (r < 1 || r > 4096) return fail(MH_ERR_ARG, "%s: bin factor %u outside 1..4096", who, r);
    if (t0 > t1 || t1 > p->h.max_T)
        return fail(MH_ERR_ARG, "%s: [%llu, %llu) is not a range inside [0, %llu)", who, (unsigned long long)t0,
                    (unsigned long long)t1, (unsigned long long)p->h.max_T);
    if (t0 % r) return fail(MH_ERR_ARG, "%s: t0 = %llu is not a multiple of the bin factor %u", who, (unsigned long long)t0, r);
    const uint32_t C = p->h.info.C;
    for (uint32_t i = 0; i < n_sel; ++i)
        if (sel[i] >= C) return fail(MH_ERR_ARG, "%s: sel[%u] = %u, the plan has %u channels", who, i, sel[i], C);
    const uint64_t nb = (t1 - t0 + r - 1) / r;
    if (n_sel > 1 && out_pitch < nb)
        return fail(MH_ERR_ARG, "%s: out_pitch %llu below the row length %llu", who, (unsigned long long)out_pitch,
                    (unsigned long long)nb);
    *empty = n_sel == 0 || nb == 0;
    if (*empty) return MH_OK;
    if (!payload || !seg_off || !peak || !enc || !out) return fail(MH_ERR_ARG, "%s: NULL argument", who);
    return check_device(p->device, who);
}

// The cache's fill records, launch(grid, first record), in the grids of mh_launch.hpp (per_block elements per workgroup
// and pass).
extern "C++" template <class Launch>
static int launch_fills(const ListCache &c, uint64_t per_block, Launch launch)
{
    const unsigned nx = mh::fill_grid_x(c.w.max_fill, per_block);
    const auto *d_fill = reinterpret_cast<const mh::RangeFill *>(c.fills());
    for (size_t f = 0; f < c.w.nfill; f += mh::kFillMaxRecords) {
        launch(dim3(nx, mh::fill_grid_y(c.w.nfill, f)), d_fill + f);
        MH_HIP(hipGetLastError());
    }
    return MH_OK;
}

int mh_decode_range(mh_plan *p, const uint32_t *payload, uint64_t payload_words, const uint64_t *seg_off,
                    const uint32_t *sel, uint32_t n_sel, uint64_t t0, uint64_t t1, const uint8_t *peak, const uint8_t *enc,
                    uint8_t *out, uint64_t out_pitch, void *stream)
{
    bool empty;
    int rc = check_range_call("mh_decode_range", p, payload, seg_off, sel, n_sel, t0, t1, 1u, peak, enc, out, out_pitch, &empty);
    if (rc || empty) return rc;
    hipStream_t st = (hipStream_t)stream;
    ListCache &c = p->range;
    if (!c.same_query(sel, n_sel, t0, t1, 0u, out_pitch) &&
        (rc = upload_list(c, mh::range_work_list(p->h, sel, n_sel, t0, t1, out_pitch), MH_CHUNK, sel, n_sel, t0, t1, 0u, out_pitch, st)))
        return rc;
    rc = launch_fills(c, 256 * 16 * 4, [&](dim3 grid, const mh::RangeFill *fill) {  // 64 KiB per workgroup and pass
        hipLaunchKernelGGL(mh::k_range_fill, grid, dim3(256), 0, st, out, fill);
    });
    if (rc || c.w.nwg == 0) return rc;
    mh::RangeArgs r{};
    r.a = decode_args(p, payload, payload_words, seg_off, peak, enc, out);
    r.task = reinterpret_cast<const mh::RangeTask *>(c.d_list);
    r.wg = reinterpret_cast<const mh::RangeWg *>(c.wgs());
    r.out = out;
    r.scratch = c.d_aux;
    return launch(p->k_range, (uint32_t)c.w.nwg, &r, st);
}

// the two output forms of mh_decode_rebin around its decoder: zero fills in front, fix-ups of the shared bins behind
extern "C++" template <class T>
static int decode_rebin(const mh_plan *p, const mh::RebinArgs &a, bool sat, hipStream_t st)
{
    const ListCache &c = p->rebin;
    T *out = static_cast<T *>(a.out);
    int rc = launch_fills(c, 256 * 16, [&](dim3 grid, const mh::RangeFill *fill) {
        hipLaunchKernelGGL(mh::k_rebin_fill<T>, grid, dim3(256), 0, st, out, fill);
    });
    if (rc || c.w.nwg == 0) return rc;
    if (c.w.naux) MH_HIP(hipMemsetAsync(c.d_aux, 0, c.w.naux * sizeof(uint32_t), st));
    if ((rc = launch(sat ? p->k_rebin_sat : p->k_rebin_wide, (uint32_t)c.w.nwg, &a, st)) || c.w.nfix == 0) return rc;
    hipLaunchKernelGGL(mh::k_rebin_fix<T>, dim3((unsigned)((c.w.nfix + 255) / 256)), dim3(256), 0, st, out,
                       reinterpret_cast<const mh::RebinFix *>(c.fixes()), (uint32_t)c.w.nfix, a.side);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

int mh_decode_rebin(mh_plan *p, const uint32_t *payload, uint64_t payload_words, const uint64_t *seg_off,
                    const uint32_t *sel, uint32_t n_sel, uint64_t t0, uint64_t t1, uint32_t r, int saturate,
                    const uint8_t *peak, const uint8_t *enc, void *out, uint64_t out_pitch, void *stream)
{
    bool empty;
    int rc = check_range_call("mh_decode_rebin", p, payload, seg_off, sel, n_sel, t0, t1, r, peak, enc, out, out_pitch, &empty);
    if (rc || empty) return rc;
    hipStream_t st = (hipStream_t)stream;
    ListCache &c = p->rebin;
    if (!c.same_query(sel, n_sel, t0, t1, r, out_pitch) &&
        (rc = upload_list(c, mh::rebin_work_list(p->h, sel, n_sel, t0, t1, r, out_pitch), sizeof(uint32_t), sel, n_sel, t0, t1, r,
                          out_pitch, st)))
        return rc;
    mh::RebinArgs a{};
    a.a = decode_args(p, payload, payload_words, seg_off, peak, enc, nullptr);
    a.task = reinterpret_cast<const mh::RebinTask *>(c.d_list);
    a.wg = reinterpret_cast<const mh::RangeWg *>(c.wgs());
    a.out = out;
    a.side = reinterpret_cast<uint32_t *>(c.d_aux);
    a.r = r;
    a.rmagic = r > 1 ? (uint32_t)((1ull << 32) / r) + 1u : 0u;
    return saturate ? decode_rebin<uint8_t>(p, a, true, st) : decode_rebin<uint32_t>(p, a, false, st);
}

int mh_validate_stream(const uint64_t *ch_len, uint32_t C, uint32_t S, uint32_t h, uint32_t mode, uint32_t window,
                       const uint8_t *sclv, uint32_t K, uint32_t seg_chunks, const uint32_t *payload,
                       uint64_t payload_words, const uint64_t *seg_words, uint64_t n_segments,
                       const uint8_t *peak, const uint8_t *enc)
{
    if (!ch_len || !sclv || !payload || !seg_words || !peak || !enc)
        return fail(MH_ERR_ARG, "mh_validate_stream: NULL argument");
    mh::PlanHost H;
    mh::Msg m;
    int rc = mh::stored_plan_host(m, "mh_validate_stream", ch_len, C, S, h, mode, window, sclv, K, seg_chunks, n_segments, H);
    if (!rc) rc = mh::validate_stream(m, H, payload, payload_words, seg_words, peak, enc);
    return rc ? fail(rc, m) : MH_OK;
}

int mh_validate_segments(const uint64_t *ch_len, uint32_t C, uint32_t S, uint32_t h, uint32_t mode, uint32_t window,
                         const uint8_t *sclv, uint32_t K, uint32_t seg_chunks, const uint32_t *payload, uint64_t payload_words,
                         const uint64_t *seg_off, const uint64_t *seg_words, uint64_t n_segments, const uint64_t *seg_idx,
                         uint64_t n_idx, const uint8_t *peak, const uint8_t *enc)
{
    if (!ch_len || !sclv || !seg_off || !seg_words || !peak || !enc || (n_idx && (!payload || !seg_idx)))
        return fail(MH_ERR_ARG, "mh_validate_segments: NULL argument");
    mh::PlanHost H;
    mh::Msg m;
    int rc = mh::stored_plan_host(m, "mh_validate_segments", ch_len, C, S, h, mode, window, sclv, K, seg_chunks, n_segments, H);
    if (!rc) rc = mh::validate_segments(m, "mh_validate_segments", H, payload, payload_words, seg_off, seg_words, seg_idx, n_idx, peak, enc);
    return rc ? fail(rc, m) : MH_OK;
}

int mh_compact(mh_plan *p, const uint32_t *payload, const uint64_t *seg_words, uint32_t *dense,
               uint64_t dense_cap_words, uint64_t *dense_off, uint64_t *total_words, void *stream)
{
    if (!p || !payload || !seg_words || !dense || !dense_off || !total_words)
        return fail(MH_ERR_ARG, "mh_compact: NULL argument");
    if (int rc_ = check_device(p->device, "mh_compact")) return rc_;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t nseg = p->h.info.n_segments;
    const unsigned scan_blocks = mh::compact_scan_blocks(nseg), groups = mh::compact_groups(nseg);
    if (scan_blocks <= 1) {  // one launch: every wave scans for itself
        hipLaunchKernelGGL(mh::k_compact<true>, dim3(groups), dim3(256), 0, st, payload,
                           (const uint64_t *)p->d_seg_off, seg_words, dense_off, dense, dense_cap_words, nseg, total_words);
        MH_HIP(hipGetLastError());
        return MH_OK;
    }
    hipLaunchKernelGGL(mh::k_scan_block_sums, dim3(scan_blocks), dim3(256), 0, st, seg_words, nseg, p->d_scan);
    hipLaunchKernelGGL(mh::k_scan_top, dim3(1), dim3(1024), 0, st, p->d_scan, (uint64_t)scan_blocks, total_words);
    hipLaunchKernelGGL(mh::k_scan_apply, dim3(scan_blocks), dim3(256), 0, st, seg_words, nseg,
                       (const uint64_t *)p->d_scan, dense_off);
    MH_HIP(hipGetLastError());
    hipLaunchKernelGGL(mh::k_compact<false>, dim3(groups), dim3(256), 0, st, payload,
                       (const uint64_t *)p->d_seg_off, seg_words, dense_off, dense, dense_cap_words, nseg, total_words);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

int mh_synth_poisson(uint8_t *data, const uint64_t *ch_off, const uint64_t *ch_len, uint32_t C,
                     uint64_t max_len, const uint32_t *thr, uint64_t seed, void *stream)
{
    if (!data || !ch_off || !ch_len || !thr || C == 0) return fail(MH_ERR_ARG, "mh_synth_poisson: bad argument");
    const mh::GridXY g = mh::synth_grid(max_len, C);
    hipLaunchKernelGGL(mh::k_synth, dim3(g.x, g.y), dim3(256), 0, (hipStream_t)stream, data,
                       ch_off, ch_len, C, thr, seed);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

int mh_rebin(const uint8_t *data, const uint64_t *in_off, const uint64_t *in_len, uint32_t C,
             uint64_t max_len, uint32_t r, int saturate, void *out, const uint64_t *out_off,
             void *stream)
{
    if (!data || !in_off || !in_len || !out || !out_off || C == 0 || r == 0)
        return fail(MH_ERR_ARG, "mh_rebin: bad argument");
    if (r > 4096) return fail(MH_ERR_ARG, "mh_rebin: r=%u above 4096", r);
    if (r >= 4) {
        const mh::Rebin3Launch l = mh::rebin3_launch(max_len, C, r);
#define MH_REBIN3(SAT_, R_)                                                                                      \
    hipLaunchKernelGGL((mh::k_rebin3<SAT_, R_>), dim3(l.grid.x, l.grid.y), dim3(256), 0, (hipStream_t)stream, \
                       data, in_off, in_len, C, r, l.g, l.u, l.upt, l.tpw, out, out_off)
#define MH_REBIN3_R(R_)               \
    do {                              \
        if (saturate)                 \
            MH_REBIN3(true, R_);      \
        else                          \
            MH_REBIN3(false, R_);     \
    } while (0)
        switch (r) {  // the reference's bin periods get straight-line kernels
        case 5: MH_REBIN3_R(5); break;
        case 10: MH_REBIN3_R(10); break;
        case 20: MH_REBIN3_R(20); break;
        case 50: MH_REBIN3_R(50); break;
        case 100: MH_REBIN3_R(100); break;
        default: MH_REBIN3_R(0); break;
        }
#undef MH_REBIN3_R
#undef MH_REBIN3
        MH_HIP(hipGetLastError());
        return MH_OK;
    }
    const mh::GridXY g = mh::rebin2_grid(max_len, C, r);
    if (saturate)
        hipLaunchKernelGGL(mh::k_rebin2<true>, dim3(g.x, g.y), dim3(256), 0, (hipStream_t)stream,
                           data, in_off, in_len, C, r, out, out_off);
    else
        hipLaunchKernelGGL(mh::k_rebin2<false>, dim3(g.x, g.y), dim3(256), 0, (hipStream_t)stream,
                           data, in_off, in_len, C, r, out, out_off);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

// the one-dimensional grid of the transposing kernels (mh_launch.hpp)
static int transposed_grid(const char *who, uint64_t T, uint32_t C, uint32_t tpw, unsigned *grid)
{
    mh::Msg m;
    const int rc = mh::transposed_grid(m, who, T, C, tpw, grid);
    return rc ? fail(rc, m) : MH_OK;
}

int mh_deinterleave(const uint8_t *in, uint64_t T, uint32_t C, uint8_t *out, const uint64_t *out_off,
                    void *stream)
{
    if (!in || !out || !out_off || C == 0) return fail(MH_ERR_ARG, "mh_deinterleave: bad argument");
    if (T == 0) return MH_OK;
    const uint32_t tpw = 4;
    unsigned grid;
    if (int rc_ = transposed_grid("mh_deinterleave", T, C, tpw, &grid)) return rc_;
    hipLaunchKernelGGL(mh::k_deinterleave2, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, T, C, tpw,
                       out, out_off);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

int mh_deinterleave_packed(const uint8_t *in, uint64_t T, uint32_t C, uint32_t bits, uint8_t *out,
                           const uint64_t *out_off, uint64_t chunk_stride, void *stream)
{
    if (!in || !out || !out_off || C == 0) return fail(MH_ERR_ARG, "mh_deinterleave_packed: bad argument");
    if (bits != 4 && bits != 2) return fail(MH_ERR_ARG, "mh_deinterleave_packed: bits=%u (4 or 2)", bits);
    if (!mh::chunk_stride_ok(chunk_stride, bits))
        return fail(MH_ERR_ARG, "mh_deinterleave_packed: chunk_stride=%llu", (unsigned long long)chunk_stride);
    if (T == 0) return MH_OK;
    const uint32_t tpw = bits == 2 ? (uint32_t)mh::P2<2>::kTpw : (uint32_t)mh::P2<4>::kTpw;  // tiles of a visit held in LDS
    unsigned grid;
    if (int rc_ = transposed_grid("mh_deinterleave_packed", T, C, tpw, &grid)) return rc_;
    // pieces that fit the Infinity Cache (256 MiB) stay cacheable for the encoder that reads them next
    const uint32_t cached = (double)T * C * bits / 8.0 <= 192.0 * 1048576.0 ? 1u : 0u;
    if (bits == 4)
        hipLaunchKernelGGL(mh::k_deinterleave_p<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, T, C, tpw,
                           out, out_off, chunk_stride, cached);
    else
        hipLaunchKernelGGL(mh::k_deinterleave_p<2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, T, C, tpw,
                           out, out_off, chunk_stride, cached);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

int mh_interleave(const uint8_t *in, const uint64_t *in_off, uint64_t T, uint32_t C, uint8_t *out, void *stream)
{
    if (!in || !in_off || !out || C == 0) return fail(MH_ERR_ARG, "mh_interleave: bad argument");
    if (T == 0) return MH_OK;
    const uint32_t tpw = 4;
    unsigned grid;
    if (int rc_ = transposed_grid("mh_interleave", T, C, tpw, &grid)) return rc_;
    hipLaunchKernelGGL(mh::k_interleave, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, in_off, T, C,
                       tpw, out);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

int mh_interleave_packed(const uint8_t *in, const uint64_t *in_off, uint64_t T, uint32_t C, uint32_t bits,
                         uint64_t chunk_stride, uint8_t *out, void *stream)
{
    if (!in || !in_off || !out || C == 0) return fail(MH_ERR_ARG, "mh_interleave_packed: bad argument");
    if (bits != 4 && bits != 2) return fail(MH_ERR_ARG, "mh_interleave_packed: bits=%u (4 or 2)", bits);
    if (!mh::chunk_stride_ok(chunk_stride, bits))
        return fail(MH_ERR_ARG, "mh_interleave_packed: chunk_stride=%llu", (unsigned long long)chunk_stride);
    if (T == 0) return MH_OK;
    const uint32_t tpw = 4;
    unsigned grid;
    if (int rc_ = transposed_grid("mh_interleave_packed", T, C, tpw, &grid)) return rc_;
    const uint32_t nt = 1u;  // non-temporal row stores, as k_interleave (profiles/r04_stream_decode.txt)
    if (bits == 4)
        hipLaunchKernelGGL(mh::k_interleave_p<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, in_off, T,
                           C, tpw, chunk_stride, nt, out);
    else
        hipLaunchKernelGGL(mh::k_interleave_p<2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, in_off, T,
                           C, tpw, chunk_stride, nt, out);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

int mh_sweep_destroy(mh_sweep *w)
{
    delete w;
    return MH_OK;
}

int mh_sweep_create(mh_sweep **sweep, const uint64_t *ch_off, const uint64_t *ch_len, uint32_t C,
                    const uint32_t *hist_bits, uint32_t nh)
{
    if (!sweep || !ch_off || !ch_len || !hist_bits) return fail(MH_ERR_ARG, "mh_sweep_create: NULL argument");
    *sweep = nullptr;
    mh::Msg m;
    if (int rc = mh::sweep_check_args(m, ch_len, C, hist_bits, nh)) return fail(rc, m);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(MH_ERR_NO_DEVICE, "no HIP device visible (libmuahuff has no CPU fallback)");
    int dev = 0;
    MH_HIP(hipGetDevice(&dev));
    mh_sweep *w = new (std::nothrow) mh_sweep;
    if (!w) return fail(MH_ERR_ARG, "out of host memory");
    w->device = dev;
    mh::SweepHost h;
    mh::sweep_host_build(h, ch_off, ch_len, C, hist_bits, nh);
    w->ni = h.ni;
    w->n_tiles = h.tile_ch.size();
    w->n_slots = h.slot_len.size();
    const mh::SweepArena a = mh::sweep_arena(h);
    w->bounds = std::move(h.bounds);  // (not a table: what mh_sweep_info reports)
    if (int rc = w->arena.create(a)) {
        mh_sweep_destroy(w);
        return rc;
    }
    const DeviceArena &d = w->arena;
    d.view(w->d_ch_off, a.ch_off), d.view(w->d_tile_ch, a.tile_ch), d.view(w->d_tile_n, a.tile_n), d.view(w->d_tile_slot, a.tile_slot);
    d.view(w->d_tile_start, a.tile_start), d.view(w->d_slot_len, a.slot_len), d.view(w->d_scratch, a.hist);
    *sweep = w;
    return MH_OK;
}

int mh_sweep_info(const mh_sweep *w, uint32_t *n_intervals, uint64_t *bounds)
{
    if (!w) return fail(MH_ERR_ARG, "mh_sweep_info: NULL sweep");
    if (n_intervals) *n_intervals = w->ni;
    if (bounds) memcpy(bounds, w->bounds.data(), w->bounds.size() * sizeof(uint64_t));
    return MH_OK;
}

int mh_sweep_run(mh_sweep *w, const uint8_t *data, uint64_t *hist, void *stream)
{
    if (!w || !data || !hist) return fail(MH_ERR_ARG, "mh_sweep_run: NULL argument");
    if (int rc_ = check_device(w->device, "mh_sweep_run")) return rc_;
    hipStream_t st = (hipStream_t)stream;
    MH_HIP(hipMemsetAsync(w->d_scratch, 0, (size_t)w->n_slots * mh::kHistStride * sizeof(unsigned long long), st));
    if (w->n_tiles) {
        const mh::HistArgs a = hist_args(data, w->d_ch_off, w->d_tile_ch, w->d_tile_start, w->d_tile_n, w->d_scratch, w->d_tile_slot);
        hipLaunchKernelGGL(mh::k_hist2<4>, dim3((unsigned)w->n_tiles), dim3(256), 0, st, a, (uint32_t)MH_SWEEP_BINS);
        MH_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(mh::k_sweep_finalize, dim3((unsigned)((w->n_slots + 255) / 256)), dim3(256), 0, st,
                       (const unsigned long long *)w->d_scratch, (const uint64_t *)w->d_slot_len,
                       (uint32_t)w->n_slots, hist);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

int mh_power_draws(const double *br, uint32_t n_br, const int32_t *idx, uint32_t Z, uint64_t n_draws,
                   double comm_energy, double per_channels, double static_power, double *x, uint64_t x_stride,
                   void *stream)
{
    if (!br || !idx || !x || n_br == 0 || x_stride == 0) return fail(MH_ERR_ARG, "mh_power_draws: bad argument");
    if (n_draws == 0) return MH_OK;
    mh::Msg m;
    unsigned grid;
    if (int rc = mh::per_item_grid(m, "mh_power_draws", "draws", n_draws, &grid)) return fail(rc, m);
    hipLaunchKernelGGL(mh::k_power_draws, dim3(grid), dim3(256), 0, (hipStream_t)stream, br,
                       idx, Z, n_draws, comm_energy, per_channels, static_power, x, x_stride);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

int mh_reduce_rows(const double *vals, const uint64_t *row_off, uint64_t n_rows, double *sum, double *mx, void *stream)
{
    if (!vals || !row_off || !sum || !mx) return fail(MH_ERR_ARG, "mh_reduce_rows: NULL argument");
    if (n_rows == 0) return MH_OK;
    mh::Msg m;
    unsigned grid;
    if (int rc = mh::per_item_grid(m, "mh_reduce_rows", "rows", n_rows, &grid)) return fail(rc, m);
    hipLaunchKernelGGL(mh::k_reduce_rows, dim3(grid), dim3(256), 0, (hipStream_t)stream, vals,
                       row_off, n_rows, sum, mx);
    MH_HIP(hipGetLastError());
    return MH_OK;
}

}  // extern "C"
#pragma GCC visibility pop
