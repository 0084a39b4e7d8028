// crossclr_api.cpp -- the extern "C" boundary declared in include/crossclr.h.
// Built by hipcc for gfx950 into libcrossclr_hip.so (the product).  The same file is built by the
// host clang with -DCROSSCLR_EMU into tests/emu/libcrossclr_emu.so, where "launch" means running
// the kernel source lane by lane on CPU threads -- test infrastructure only.
#include "../../include/crossclr.h"
#include "crossclr_kernels_generic.h"
#include "crossclr_kernels_hvp.h"
#include "crossclr_kernels_topk.h"
#include "crossclr_kernels_hardneg.h"
#include "crossclr_kernels_infonce.h"
#include "crossclr_kernels_sigmoid.h"
#include "crossclr_kernels_pairids.h"
#include "crossclr_kernels_fast.h"
#include "crossclr_kernels_project.h"
#include "crossclr_kernels_saved32.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#ifndef CROSSCLR_DEFAULT_BWD_KERNEL
#define CROSSCLR_DEFAULT_BWD_KERNEL 1   // 1: 32-row waves, 2: 16-row waves (for Dpad <= 512, where both exist)
#endif

using namespace crossclr;

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// which kernel template the most recent forward (0) / gradient-product (1) / row-kernel (2: normalisation and lay-out, gradient finish) launch
// of this process went to (crossclr_last_kernel; pointers to string literals, written whole: a reader on another thread -- autograd runs
// backward() on its own -- sees the old or the new name)
static const char* volatile g_last_kernel[3] = {"", "", ""};
namespace crossclr {
void note_kernel(int which, const char* name) { g_last_kernel[which == 2 ? 2 : (which & 1)] = name; }
}  // namespace crossclr
static void note_generic_launch(const char* what) {      // (the generic kernels are launched from this file: their launch_status label names them)
    if (!strncmp(what, "fwd_sums_kernel", 15)) crossclr::note_kernel(0, what);
    else if (!strncmp(what, "bwd_kernel", 10) || !strncmp(what, "bwd_saved32_kernel", 18) || !strncmp(what, "bwd_saved_x3_kernel", 19))
        crossclr::note_kernel(1, what);
    else if (!strncmp(what, "normalize_", 10) || !strcmp(what, "topk_pack_kernel") || !strncmp(what, "bwd_finish_", 11) ||
             !strcmp(what, "pairloss_backward_finish_kernel") || !strcmp(what, "hardneg_backward_kernel"))
        crossclr::note_kernel(2, what);
}

#ifdef CROSSCLR_EMU
#define LAUNCH(kernel, grid, block, stream, ...) emu::launch(kernel, grid, block, __VA_ARGS__)
static int launch_status(const char* what) { note_generic_launch(what); return CROSSCLR_OK; }
#else
#define LAUNCH(kernel, grid, block, stream, ...) \
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)(stream), __VA_ARGS__)
static int launch_status(const char* what) {
    note_generic_launch(what);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CROSSCLR_E_HIP, "%s: %s", what, hipGetErrorString(e));
    return CROSSCLR_OK;
}
#endif

extern "C" int crossclr_abi_version(void) { return CROSSCLR_ABI_VERSION; }
extern "C" const char* crossclr_last_error(void) { return g_err; }
extern "C" const char* crossclr_last_kernel(int which) { return g_last_kernel[which == 2 ? 2 : (which & 1)]; }
extern "C" const char* crossclr_backend(void) {
#ifdef CROSSCLR_EMU
    return "emu-host";
#else
    return "hip-gfx950";
#endif
}

static int round_up(int x, int m) { return (x + m - 1) / m * m; }
// CROSSCLR_MODE_BF16X3 (include/crossclr.h): the generic kernels of the fp32 mode on the split operand (x3_t)
static bool is_x3(const crossclr_plan* p) { return p->mode == CROSSCLR_MODE_BF16X3; }
static int refuse_x3(const char* what) {
    return fail(CROSSCLR_E_ARG, "%s: CROSSCLR_MODE_BF16X3 plans are not supported here (single-device loss step only)", what);
}
// label of a generic launch (crossclr_last_kernel): the split-operand instantiations carry <x3_t>
template <typename T> static const char* glabel(const char* plain, const char* x3) { return std::is_same<T, x3_t>::value ? x3 : plain; }
static const float* const kNoF = nullptr;     // (kernel arguments a launch does not use)
// the packed operand's element type from plan->mode -- f(type_tag<float>()), f(type_tag<x3_t>()) or f(type_tag<bf16_t>()); SPLIT = false:
// entry points without split-operand kernels (they refuse CROSSCLR_MODE_BF16X3 before they get here): float or bf16_t only
template <typename T> struct type_tag { using type = T; };
template <bool SPLIT = true, class F> static int with_plan_type(const crossclr_plan* plan, F f) {
    if (plan->mode == CROSSCLR_MODE_FP32) return f(type_tag<float>());
    if constexpr (SPLIT) if (is_x3(plan)) return f(type_tag<x3_t>());
    return f(type_tag<bf16_t>());
}
// the caller's element type from in_dtype -- f(type_tag<float>()), <double>, <in_f16> or <in_bf16>
template <class F> static int with_in_dtype(int in_dtype, F f) {
    switch (in_dtype) {
        case CROSSCLR_IN_F32: return f(type_tag<float>());
        case CROSSCLR_IN_F64: return f(type_tag<double>());
        case CROSSCLR_IN_F16: return f(type_tag<in_f16>());
        case CROSSCLR_IN_BF16: return f(type_tag<in_bf16>());
    }
    return fail(CROSSCLR_E_ARG, "bad in_dtype %d", in_dtype);
}
// D columns per thread block: the first of DCS... that divides Dpad (the last one, 64, always does) -- f(std::integral_constant<int, DC>())
template <int DC, int... REST, class F> static void with_d_chunk(int Dpad, F f) {
    if constexpr (sizeof...(REST) == 0) f(std::integral_constant<int, DC>());
    else if (Dpad % DC == 0) f(std::integral_constant<int, DC>());
    else with_d_chunk<REST...>(Dpad, f);
}

// tuning knobs from the environment, read ONCE per process (not per call: crossclr_make_plan sits on the step's host path)
struct EnvKnobs {
    bool disable_fast, disable_symmetric, disable_save, disable_xf;
    int bwd_kernel, fwd_blocks, bwd_slices;
    EnvKnobs() {
        disable_fast = getenv("CROSSCLR_DISABLE_FAST") != nullptr;
        disable_symmetric = getenv("CROSSCLR_DISABLE_SYMMETRIC") != nullptr;
        disable_save = getenv("CROSSCLR_DISABLE_SAVE") != nullptr;
        disable_xf = getenv("CROSSCLR_DISABLE_XF") != nullptr;  // no fragment-major operand copy: the saved backward stages the column tiles through LDS
        const char* e = getenv("CROSSCLR_BWD_KERNEL");
        bwd_kernel = e ? atoi(e) : 0;
        e = getenv("CROSSCLR_FWD_BLOCKS");
        fwd_blocks = e ? atoi(e) : 0;
        e = getenv("CROSSCLR_BWD_SLICES");
        bwd_slices = e ? atoi(e) : 0;
    }
};
static const EnvKnobs& env_knobs() {
#ifdef CROSSCLR_EMU
    static thread_local EnvKnobs k;   // the CPU tests flip these variables between calls (monkeypatch): re-read there
    k = EnvKnobs();
    return k;
#else
    static const EnvKnobs k;
    return k;
#endif
}

// forward workspace ("part") layout, in floats:
//   [4 launch groups][fwd_slots][2*bpad] | colpart (symmetric launch) [<= 2*bpad/128 row blocks][2*bpad]
//   | colpart (pairs launch) [row blocks][(world-1)/2 ranks * 2*bpad] | header [4][4] ints
// (the symmetric launch's column sums are read by the finish kernel, so the pairs launch needs its own region)
static const int kLaunchGroups = CROSSCLR_LAUNCH_GROUPS;
static size_t ws_colpart_off(const crossclr_plan* p) { return (size_t)kLaunchGroups * p->fwd_slots * 2 * p->bpad; }
static size_t ws_colpart_rows(const crossclr_plan* p) { return (size_t)(2 * p->bpad / 128 + 1); }
static size_t ws_paircol_off(const crossclr_plan* p) { return ws_colpart_off(p) + ws_colpart_rows(p) * 2 * p->bpad; }
static size_t ws_flag_off(const crossclr_plan* p) {
    const size_t k = p->world > 2 ? (size_t)(p->world - 1) / 2 : 0;
    return ws_paircol_off(p) + ws_colpart_rows(p) * k * 2 * p->bpad;
}

static int device_zero(void* where, size_t bytes, void* stream) {
#ifdef CROSSCLR_EMU
    (void)stream;
    memset(where, 0, bytes);
    return CROSSCLR_OK;
#else
    hipError_t e = hipMemsetAsync(where, 0, bytes, (hipStream_t)stream);
    if (e != hipSuccess) return fail(CROSSCLR_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    return CROSSCLR_OK;
#endif
}
static int device_zero_header(int* where, void* stream) {  // kind 0 = dense slots (generic kernels)
#ifdef CROSSCLR_EMU
    (void)stream;
    memset(where, 0, 16);
    return CROSSCLR_OK;
#else
    hipError_t e = hipMemsetAsync(where, 0, 16, (hipStream_t)stream);
    if (e != hipSuccess) return fail(CROSSCLR_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    return CROSSCLR_OK;
#endif
}
// one launch group of the forward workspace: its partial sums, its header, and the two column-partial regions (shared by the groups)
struct FwdSlot { float* out; int* header; float* colpart; float* paircol; };
static FwdSlot fwd_group(const crossclr_plan* plan, float* part, int group) {
    return {part + (size_t)group * plan->fwd_slots * 2 * plan->bpad, reinterpret_cast<int*>(part + ws_flag_off(plan)) + 4 * group,
            part + ws_colpart_off(plan), part + ws_paircol_off(plan)};
}
static int fwd_slot(const crossclr_plan* plan, float* part, int slot0, FwdSlot* s) {
    if (plan->fwd_slots <= 0 || slot0 < 0 || slot0 % plan->fwd_slots != 0 || slot0 / plan->fwd_slots >= kLaunchGroups)
        return fail(CROSSCLR_E_ARG, "slot0 must be L * plan->fwd_slots, L = 0..%d", kLaunchGroups - 1);
    *s = fwd_group(plan, part, slot0 / plan->fwd_slots);
    return CROSSCLR_OK;
}

extern "C" int crossclr_make_plan(int b, int D, int world, int rank, int mode, crossclr_plan* plan) {
    if (!plan) return fail(CROSSCLR_E_ARG, "plan is NULL");
    if (b < 1 || D < 1) return fail(CROSSCLR_E_ARG, "need b >= 1 and D >= 1 (got b=%d D=%d)", b, D);
    if (world < 1 || rank < 0 || rank >= world) return fail(CROSSCLR_E_ARG, "bad world/rank %d/%d", world, rank);
    if (mode != CROSSCLR_MODE_FP32 && mode != CROSSCLR_MODE_BF16 && mode != CROSSCLR_MODE_BF16X3) return fail(CROSSCLR_E_ARG, "bad mode %d", mode);
    if (mode == CROSSCLR_MODE_BF16X3 && world != 1)
        return fail(CROSSCLR_E_ARG, "CROSSCLR_MODE_BF16X3 is single-device: world must be 1 (got %d)", world);
    // the forward's flat work list, the stash and the column-sum workspace are indexed with 32-bit integers:
    // (2b/128 row blocks) x (2B/32 column tiles) must stay below 2^31 (whichever kernel the plan ends up with)
    {
        const long long bp = ((long long)b + kRowPad - 1) / kRowPad * kRowPad;
        const long long items = (2 * bp / 128) * (2 * bp * world / 32);
        if ((long long)b * world > (1 << 21) || items >= (1LL << 31))
            return fail(CROSSCLR_E_ARG, "batch too large: b=%d x world=%d gives %lld work items (limit 2^31; global rows limit 2^21)", b, world, items);
    }
    memset(plan, 0, sizeof(*plan));
    plan->b = b; plan->D = D; plan->world = world; plan->rank = rank; plan->mode = mode;
    plan->bpad = round_up(b, kRowPad);
    plan->fast_path = 0;
    int dpad = round_up(D, 64);
    const EnvKnobs& env = env_knobs();
    if (mode == CROSSCLR_MODE_BF16 && !env.disable_fast) {  // env knob: A/B against the generic path
        int fp = fast_dpad(D);
        if (fp > 0) { dpad = fp; plan->fast_path = 1; }
    }
    if (!plan->fast_path && dpad > 256) dpad = round_up(D, 256);  // generic backward slices D by 256
    // wide bf16 plans (1024 < D <= 8192): generic forward, but its exponentials are saved for the D-slice backward, which runs as 3 ... 16
    // column parts of 384 / 512 columns -- the operand is padded to parts x columns
    bool wide = false;
    if (mode == CROSSCLR_MODE_BF16 && !plan->fast_path && !env.disable_fast && !env.disable_save && !env.disable_symmetric && wide_bf16_dpad(D) > 0) {
        dpad = wide_bf16_dpad(D);
        wide = true;
    }
    plan->Dpad = dpad;
    // backward kernel: 0 generic tiled, 1 register-resident 32-row waves (Dpad <= 512), 2 16-row waves (Dpad <= 1024)
    plan->fast_bwd = 0;
    if (mode == CROSSCLR_MODE_BF16 && !env.disable_fast) {
        if (plan->fast_path) plan->fast_bwd = dpad <= 512 ? CROSSCLR_DEFAULT_BWD_KERNEL : 2;
        if (env.bwd_kernel == 16 && plan->fast_path) plan->fast_bwd = 2;              // tuning knob: 16 or 32
        if (env.bwd_kernel == 32 && plan->fast_path && dpad <= 512) plan->fast_bwd = 1;
    }
    // forward partial-sum slots.  generic kernels: (row block x column split) grid, enough work items to
    // fill 256 CUs a few times over.  fast path: persistent blocks over a flat work list (see FwdWork);
    // a row block's slots = the thread blocks whose range touches it.
    const int row_blocks = 2 * plan->bpad / 128;
    const int col_tiles = 2 * plan->bpad / 128;  // per column rank
    int nsplit = (1024 + row_blocks - 1) / row_blocks;
    if (nsplit > col_tiles) nsplit = col_tiles;
    if (nsplit < 1) nsplit = 1;
    plan->fwd_blocks = 0;
    if (plan->fast_path) {
        plan->fwd_blocks = 256;  // one persistent block per MI355X CU (LDS-limited to one block per CU)
        if (env.fwd_blocks >= 1 && env.fwd_blocks <= 4096) plan->fwd_blocks = env.fwd_blocks;   // tuning knob
        int slots = fwd_max_slots(fast_forward_work(plan, 1, -1, true));
        int s2 = fwd_max_slots(fast_forward_work(plan, 1, -1, false));
        if (s2 > slots) slots = s2;
        if (world > 1) {
            int s3 = fwd_max_slots(fast_forward_work(plan, world, 0, false));
            if (s3 > slots) slots = s3;
        }
        if (world > 2) {   // crossclr_forward_pairs over (world-1)/2 ranks
            int s4 = fwd_max_slots(fast_forward_work(plan, (world - 1) / 2, -1, false, true));
            if (s4 > slots) slots = s4;
        }
        nsplit = slots;
    }
    plan->fwd_slots = nsplit;
    plan->fwd_ws_floats = 0;  // set below
    // backward column slices: each slice walks its share of the column tiles and writes its own gradient
    // slice (summed by crossclr_backward_finish): enough thread blocks to occupy 256 CUs, >= 2 tiles each
    {
        const int tile = plan->fast_bwd ? 32 : 64;
        int row_blk = 64;
        if (plan->fast_bwd) row_blk = fast_bwd_rows_per_block(plan->Dpad, plan->fast_bwd == 2);
        int dsl = 1;
        if (!plan->fast_bwd) dsl = plan->Dpad % 256 == 0 ? plan->Dpad / 256 : (plan->Dpad % 128 == 0 ? plan->Dpad / 128 : plan->Dpad / 64);
        const int blocks = (2 * plan->bpad / row_blk) * dsl;
        int sl = (256 + blocks - 1) / blocks;
        if (wide) {   // saved backward: (128-row blocks) x (column parts) x slices thread blocks, one per CU: the cut with the fewest rounds of 256
            const int wb = (2 * plan->bpad / 128) * (dpad / (dpad % 512 == 0 ? 512 : 384));
            double best = 1e30;
            for (int c = 1; c <= 4; ++c) {
                const double rounds = (double)((wb * c + 255) / 256) / c;
                if (rounds < best - 1e-9) { best = rounds; sl = c; }
            }
            if (wb < 256 && sl < (256 + wb - 1) / wb) sl = (256 + wb - 1) / wb;
        }
        const int tiles = 2 * plan->bpad / tile;
        if (sl > tiles / 2) sl = tiles / 2;
        if (sl > 16) sl = 16;
        if (sl < 1) sl = 1;
        if (env.bwd_slices >= 1 && env.bwd_slices <= tiles / 2 && env.bwd_slices <= 64) sl = env.bwd_slices;   // tuning knob
        plan->bwd_slices = sl;
    }
    {
        const int rows_per_block = 256 / kFinishLpr;
        int nb = (2 * plan->bpad + rows_per_block - 1) / rows_per_block;      // finish kernels: 256 / LPR rows per block, grid-stride beyond
        if (nb > 1024) nb = 1024;
        plan->loss_ws_doubles = 1 + nb;
    }
    plan->fwd_ws_floats = ws_flag_off(plan) + 4 * kLaunchGroups;   // + the launch groups' headers
    const size_t esz = mode == CROSSCLR_MODE_BF16 ? 2 : 4;      // (BF16X3: hi and lo)
    plan->operand_bytes = (size_t)2 * plan->bpad * plan->Dpad * esz;
    plan->gbuf_bytes = (size_t)plan->bwd_slices * 2 * plan->bpad * plan->Dpad * 4;
    plan->stash_bytes = 0;
    if (plan->fast_path && plan->fast_bwd && !env.disable_save) plan->stash_bytes = fast_stash_bytes(plan->bpad, plan->Dpad);
    if (wide) plan->stash_bytes = wide_stash_bytes(plan->bpad);
    if (wide && plan->stash_bytes && !env.disable_xf && plan->operand_bytes < ((size_t)1 << 32)) plan->xf_bytes = plan->operand_bytes;
    // exact-fp32 mode (and BF16X3, the same stash): the whole stacked [2 bpad] x [2 bpad] matrix of fp32 exponentials (1 GiB at b = 8192), up to 16 GiB
    if ((mode == CROSSCLR_MODE_FP32 || mode == CROSSCLR_MODE_BF16X3) && !env.disable_save && plan->operand_bytes < (1ull << 32)) {
        const size_t sb = (size_t)2 * plan->bpad * (size_t)2 * plan->bpad * 4;
        if (sb <= ((size_t)16 << 30)) plan->stash_bytes = sb;
    }
    // the fragment-major copy of the bf16 operand (crossclr_normalize_xf -> crossclr_backward_saved_xf): local block, Dpad <= 1024
    if (plan->fast_path && plan->fast_bwd && plan->stash_bytes && plan->Dpad <= 1024 && !env.disable_xf) plan->xf_bytes = plan->operand_bytes;
    return CROSSCLR_OK;
}

static bool needs_row_shift(float temperature, float negative_weight) {
    const double it = 1.0 / (double)temperature, aw = fabs((double)negative_weight);
    return it * (aw > 1.0 ? aw : 1.0) > 128.0;   // |logit| <= this bound because the rows are unit vectors
}

static int make_geo(const crossclr_plan* p, int col_ranks, int col_rank0, int skip_rank, float temperature,
                    float negative_weight, Geo* g, bool allow_row_shift = false) {
    if (!p) return fail(CROSSCLR_E_ARG, "plan is NULL");
    if (!(temperature > 0.f) || !isfinite(temperature)) return fail(CROSSCLR_E_ARG, "temperature must be > 0");
    if (!isfinite(negative_weight)) return fail(CROSSCLR_E_ARG, "negative_weight must be finite");
    if (col_ranks < 1) return fail(CROSSCLR_E_ARG, "col_ranks must be >= 1");
    g->b = p->b; g->bpad = p->bpad; g->D = p->D; g->Dpad = p->Dpad;
    g->col_ranks = col_ranks; g->col_rank0 = col_rank0; g->row_rank = p->rank; g->skip_rank = skip_rank;
    g->col_wrap = 0;
    const double it = 1.0 / (double)temperature;
    const double aw = fabs((double)negative_weight);
    const double bound = it * (aw > 1.0 ? aw : 1.0);  // |logit| <= bound because the rows are unit vectors
    // fixed soft-max shift: exp(logit - shift) must neither overflow (<= e^64 per term) nor push the
    // always-present exp(0 - shift) self term out of fp32 range (shift <= 64)
    double shift = bound > 64.0 ? bound - 64.0 : 0.0;
    g->row_shift = 0;
    if (shift > 64.0) {
        if (!allow_row_shift)
            return fail(CROSSCLR_E_RANGE, "temperature %g too small for the fixed-shift soft-max (max |logit| %g > 128): use the "
                        "two-pass entry points (crossclr_forward_rowmax + crossclr_*_s)", (double)temperature, bound);
        g->row_shift = 1;   // per-row shifts (the row maxima of crossclr_forward_rowmax) replace the common one
        shift = 0.0;
    }
    g->c_inter = (float)(it * (double)kLog2e);
    g->c_intra = (float)(it * (double)negative_weight * (double)kLog2e);
    g->m2 = (float)(shift * (double)kLog2e);
    return CROSSCLR_OK;
}

// ------------------------------------------------------------------------------------------------
template <typename TIN, bool NORM>
static int normalize_t(const crossclr_plan* p, const void* v, const void* t, long ldv, long ldt, void* xhat,
                       float* inv_norm, float* diag, void* stream, int* zero_word) {
    Geo g; memset(&g, 0, sizeof(g));
    g.b = p->b; g.bpad = p->bpad; g.D = p->D; g.Dpad = p->Dpad;
    dim3 grid((p->bpad + 3) / 4), block(256);
    return with_plan_type(p, [&](auto t_out) {
        using T = typename decltype(t_out)::type;
        LAUNCH((normalize_kernel<TIN, T, NORM>), grid, block, stream, (const TIN*)v, (const TIN*)t, ldv, ldt, g, (T*)xhat, inv_norm, diag,
               zero_word);
        return launch_status("normalize_kernel");
    });
}
template <bool NORM>
static int normalize_any(const crossclr_plan* plan, const void* video, const void* text, long ld_video, long ld_text, int in_dtype,
                         void* xhat, float* inv_norm, float* diag_cos, void* stream, int* zero_word = nullptr) {
    if (!plan || !video || !text || !xhat || !inv_norm || !diag_cos) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (ld_video < plan->D || ld_text < plan->D) return fail(CROSSCLR_E_ARG, "row stride smaller than D");
    return with_in_dtype(in_dtype, [&](auto tin) {
        return normalize_t<typename decltype(tin)::type, NORM>(plan, video, text, ld_video, ld_text, xhat, inv_norm, diag_cos, stream, zero_word);
    });
}

template <typename TIN, bool NORM>
static int normalize_xf_t(const crossclr_plan* p, const void* v, const void* t, long ldv, long ldt, void* xhat, void* xf,
                          float* inv_norm, float* diag, void* stream, int* zero_word) {
    Geo g; memset(&g, 0, sizeof(g));
    g.b = p->b; g.bpad = p->bpad; g.D = p->D; g.Dpad = p->Dpad;
    if (p->Dpad <= 512)
        LAUNCH((normalize_xf_kernel<TIN, NORM, 2>), dim3(p->bpad / 16), dim3(512), stream, (const TIN*)v, (const TIN*)t, ldv, ldt, g,
               (bf16_t*)xhat, (unsigned char*)xf, inv_norm, diag, zero_word);
    else
        LAUNCH((normalize_xf_kernel<TIN, NORM, 4>), dim3(p->bpad / 16), dim3(512), stream, (const TIN*)v, (const TIN*)t, ldv, ldt, g,
               (bf16_t*)xhat, (unsigned char*)xf, inv_norm, diag, zero_word);
    return launch_status("normalize_xf_kernel");
}
template <bool NORM>
static int normalize_xf_any(const crossclr_plan* plan, const void* video, const void* text, long ld_video, long ld_text, int in_dtype,
                            void* xhat, void* xf, float* inv_norm, float* diag_cos, void* stream, int* zero_word = nullptr) {
    if (!plan || !video || !text || !xhat || !xf || !inv_norm || !diag_cos) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (ld_video < plan->D || ld_text < plan->D) return fail(CROSSCLR_E_ARG, "row stride smaller than D");
    if (!plan->xf_bytes) return fail(CROSSCLR_E_ARG, "this plan has no fragment-major operand (xf_bytes == 0): use crossclr_normalize / crossclr_pack");
    if (plan->Dpad > 1024) {   // wide plans: the row kernel, then the packed rows re-laid fragment-major (1024 columns of a 32-row tile per block)
        if (int rc = normalize_any<NORM>(plan, video, text, ld_video, ld_text, in_dtype, xhat, inv_norm, diag_cos, stream, zero_word)) return rc;
        return crossclr_pack_xf_from_packed(plan, xhat, 1, xf, stream);
    }
    return with_in_dtype(in_dtype, [&](auto tin) {
        return normalize_xf_t<typename decltype(tin)::type, NORM>(plan, video, text, ld_video, ld_text, xhat, xf, inv_norm, diag_cos, stream, zero_word);
    });
}
extern "C" int crossclr_normalize_xf(const crossclr_plan* plan, const void* video, const void* text, long ld_video, long ld_text,
                                     int in_dtype, void* xhat, void* xhat_xf, float* inv_norm, float* diag_cos, void* stream) {
    return normalize_xf_any<true>(plan, video, text, ld_video, ld_text, in_dtype, xhat, xhat_xf, inv_norm, diag_cos, stream);
}
extern "C" int crossclr_pack_xf(const crossclr_plan* plan, const void* video_hat, const void* text_hat, long ld_video, long ld_text,
                                int in_dtype, void* xhat, void* xhat_xf, float* inv_norm, float* diag_cos, void* stream) {
    return normalize_xf_any<false>(plan, video_hat, text_hat, ld_video, ld_text, in_dtype, xhat, xhat_xf, inv_norm, diag_cos, stream);
}

extern "C" int crossclr_pack(const crossclr_plan* plan, const void* video_hat, const void* text_hat, long ld_video,
                             long ld_text, int in_dtype, void* xhat, float* inv_norm, float* diag_cos, void* stream) {
    return normalize_any<false>(plan, video_hat, text_hat, ld_video, ld_text, in_dtype, xhat, inv_norm, diag_cos, stream);
}

extern "C" int crossclr_normalize(const crossclr_plan* plan, const void* video, const void* text, long ld_video,
                                  long ld_text, int in_dtype, void* xhat, float* inv_norm, float* diag_cos,
                                  void* stream) {
    return normalize_any<true>(plan, video, text, ld_video, ld_text, in_dtype, xhat, inv_norm, diag_cos, stream);
}

// ------------------------------------------------------------------------------------------------
// producer-side fusion (crossclr_kernels_project.h)
template <typename TIN, bool WF>
static int project_pack_t(const crossclr_plan* p, const void* xv, const void* xt, long ldv, long ldt, int Din_v, int Din_t, const void* wv,
                          const void* wt, int ldw_v, int ldw_t, const float* bv, const float* bt, void* xhat, float* inv_norm, float* diag,
                          void* stream) {
    Geo g; memset(&g, 0, sizeof(g));
    g.b = p->b; g.bpad = p->bpad; g.D = p->D; g.Dpad = p->Dpad;
    // 64 rows per block up to Dpad = 512 when that still gives every CU a block; 32 rows otherwise (and always above 512: accumulators)
    const bool rows32 = p->bpad / 64 < 256;
    dim3 grid(p->bpad / 64), grid32(p->bpad / 32), block(256);
#define CROSSCLR_LPPX(DKP, RFV, GRID) LAUNCH((project_pack_kernel<TIN, DKP, RFV, WF>), GRID, block, stream, (const TIN*)xv, (const TIN*)xt, ldv, ldt, Din_v, Din_t, \
                                             (const bf16_t*)wv, (const bf16_t*)wt, ldw_v, ldw_t, bv, bt, g, (bf16_t*)xhat, inv_norm, diag)
#define CROSSCLR_LPP(DKP) do { if (rows32) CROSSCLR_LPPX(DKP, 1, grid32); else CROSSCLR_LPPX(DKP, 2, grid); } while (0)
    switch (p->Dpad) {
        case 128: CROSSCLR_LPP(1); break;
        case 256: CROSSCLR_LPP(2); break;
        case 384: CROSSCLR_LPP(3); break;
        case 512: CROSSCLR_LPP(4); break;
        case 768: CROSSCLR_LPPX(6, 1, grid32); break;        // wide embeddings: 32 rows per block (the accumulators of 64 x 1024 x 2 would not fit)
        case 1024: CROSSCLR_LPPX(8, 1, grid32); break;
        default: return fail(CROSSCLR_E_ARG, "crossclr_project_pack: Dpad %d (supported: <= 1024)", p->Dpad);
    }
#undef CROSSCLR_LPP
#undef CROSSCLR_LPPX
    return launch_status("project_pack_kernel");
}

template <bool WF>
static int project_pack_any(const crossclr_plan* plan, const void* x_video, const void* x_text, long ld_video, long ld_text,
                            int Din_video, int Din_text, int in_dtype, const void* w_video, const void* w_text, int ldw_video,
                            int ldw_text, const float* bias_video, const float* bias_text, void* xhat, float* inv_norm, float* diag_cos, void* stream) {
    if (!plan || !x_video || !x_text || !w_video || !w_text || !xhat || !inv_norm || !diag_cos) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (plan->mode != CROSSCLR_MODE_BF16 || !plan->fast_path || plan->Dpad > 1024)
        return fail(CROSSCLR_E_ARG, "crossclr_project_pack: bf16 plans with D <= 1024 only");
    if (Din_video < 1 || Din_text < 1 || ld_video < Din_video || ld_text < Din_text) return fail(CROSSCLR_E_ARG, "row stride smaller than Din");
    if (ldw_video % 64 != 0 || ldw_video < Din_video || ldw_text % 64 != 0 || ldw_text < Din_text)
        return fail(CROSSCLR_E_ARG, "weights must be zero-padded to ldw = a multiple of 64 >= Din (got %d / %d for Din %d / %d)", ldw_video, ldw_text, Din_video, Din_text);
    return with_in_dtype(in_dtype, [&](auto tin) {
        return project_pack_t<typename decltype(tin)::type, WF>(plan, x_video, x_text, ld_video, ld_text, Din_video, Din_text, w_video, w_text, ldw_video,
                                                                ldw_text, bias_video, bias_text, xhat, inv_norm, diag_cos, stream);
    });
}
extern "C" int crossclr_project_pack(const crossclr_plan* plan, const void* x_video, const void* x_text, long ld_video, long ld_text,
                                     int Din_video, int Din_text, int in_dtype, const void* w_video, const void* w_text, int ldw_video,
                                     int ldw_text, const float* bias_video,
                                     const float* bias_text, void* xhat, float* inv_norm, float* diag_cos, void* stream) {
    return project_pack_any<false>(plan, x_video, x_text, ld_video, ld_text, Din_video, Din_text, in_dtype, w_video, w_text, ldw_video, ldw_text,
                                   bias_video, bias_text, xhat, inv_norm, diag_cos, stream);
}
extern "C" int crossclr_project_pack_wf(const crossclr_plan* plan, const void* x_video, const void* x_text, long ld_video, long ld_text,
                                        int Din_video, int Din_text, int in_dtype, const void* wf_video, const void* wf_text, int ldw_video,
                                        int ldw_text, const float* bias_video,
                                        const float* bias_text, void* xhat, float* inv_norm, float* diag_cos, void* stream) {
    return project_pack_any<true>(plan, x_video, x_text, ld_video, ld_text, Din_video, Din_text, in_dtype, wf_video, wf_text, ldw_video, ldw_text,
                                  bias_video, bias_text, xhat, inv_norm, diag_cos, stream);
}

// the projection's weight gradient: split-K MFMA kernel + reduce (crossclr_kernels_project.h)
static int project_dw_splits(int b, int D, int Din_v, int Din_t) {
    const int Dp = round_up(D, 128), Dinp = round_up(Din_v > Din_t ? Din_v : Din_t, 128);
    const int tiles = 2 * (Dp / 128) * (Dinp / 128);
    int ns = (512 + tiles - 1) / tiles;                     // two thread blocks per CU: one wave per SIMD alone hides no latency
    const int max_by_rows = b / 64 > 1 ? b / 64 : 1;        // at least two 32-row chunks per split
    if (ns > max_by_rows) ns = max_by_rows;
    if (ns > 32) ns = 32;
    return ns < 1 ? 1 : ns;
}
extern "C" size_t crossclr_project_dw_ws_floats(int b, int D, int Din_video, int Din_text) {
    if (b < 1 || D < 1 || Din_video < 1 || Din_text < 1) return 0;
    const size_t Dp = round_up(D, 128), Dinp = round_up(Din_video > Din_text ? Din_video : Din_text, 128);
    const size_t ns = project_dw_splits(b, D, Din_video, Din_text);
    return 2 * ns * Dp * Dinp + 2 * ns * Dp;
}
template <typename TIN>
static int project_dw_t(int b, int D, const void* gyv, const void* gyt, long ldgy, const void* xv, const void* xt, long ldxv, long ldxt,
                        int Din_v, int Din_t, float* ws, float* dwv, float* dwt, long lddwv, long lddwt, float* dbv, float* dbt, void* stream) {
    const int Dp = round_up(D, 128), Dinp = round_up(Din_v > Din_t ? Din_v : Din_t, 128);
    const int ns = project_dw_splits(b, D, Din_v, Din_t);
    float* partial = ws;
    float* dbpart = ws + (size_t)2 * ns * Dp * Dinp;
    LAUNCH((project_dw_kernel<TIN>), dim3(2 * ns, Dp / 128, Dinp / 128), dim3(256), stream, (const in_bf16*)gyv, (const in_bf16*)gyt, ldgy,
           (const TIN*)xv, (const TIN*)xt, ldxv, ldxt, b, D, Din_v, Din_t, ns, partial, Dp, Dinp, dbpart);
    LAUNCH(project_dw_reduce_kernel, dim3((Dinp + 255) / 256, D, 2), dim3(256), stream, (const float*)partial, (const float*)dbpart, ns, D, Dp, Dinp,
           Din_v, Din_t, dwv, dwt, lddwv, lddwt, dbv, dbt);
    return launch_status("project_dw_kernel");
}
extern "C" int crossclr_project_dw(int b, int D, const void* gy_video, const void* gy_text, long ld_gy, const void* x_video, const void* x_text,
                                   long ld_xv, long ld_xt, int Din_video, int Din_text, int in_dtype, float* ws, float* dw_video, float* dw_text,
                                   long ld_dwv, long ld_dwt, float* db_video, float* db_text, void* stream) {
    if (!gy_video || !gy_text || !x_video || !x_text || !ws || !dw_video || !dw_text) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (b < 1 || D < 1 || Din_video < 1 || Din_text < 1 || ld_gy < D || ld_xv < Din_video || ld_xt < Din_text || ld_dwv < Din_video || ld_dwt < Din_text)
        return fail(CROSSCLR_E_ARG, "crossclr_project_dw: bad sizes / strides");
    return with_in_dtype(in_dtype, [&](auto tin) {
        return project_dw_t<typename decltype(tin)::type>(b, D, gy_video, gy_text, ld_gy, x_video, x_text, ld_xv, ld_xt, Din_video, Din_text, ws, dw_video,
                                                          dw_text, ld_dwv, ld_dwt, db_video, db_text, stream);
    });
}

extern "C" int crossclr_project_backward_prep(const crossclr_plan* plan, const float* g_video, const float* g_text, long ld_gv,
                                              long ld_gt, const void* xhat, const float* inv_norm, float* gy_video, float* gy_text,
                                              long ld_out, void* stream) {
    if (!plan || !g_video || !g_text || !xhat || !inv_norm || !gy_video || !gy_text) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (plan->mode != CROSSCLR_MODE_BF16) return fail(CROSSCLR_E_ARG, "crossclr_project_backward_prep: bf16 plans only");
    if (ld_gv < plan->D || ld_gt < plan->D || ld_out < plan->D) return fail(CROSSCLR_E_ARG, "row stride smaller than D");
    Geo g; memset(&g, 0, sizeof(g));
    g.b = plan->b; g.bpad = plan->bpad; g.D = plan->D; g.Dpad = plan->Dpad;
    LAUNCH(project_backward_prep_kernel, dim3((plan->b + 3) / 4), dim3(256), stream, g_video, g_text, ld_gv, ld_gt, g, (const bf16_t*)xhat,
           inv_norm, gy_video, gy_text, ld_out);
    return launch_status("project_backward_prep_kernel");
}

// ------------------------------------------------------------------------------------------------
// sample weights: both k arrays or neither (a missing struct / NULL arrays = all ones = the reference's loss)
static int unpack_k(const crossclr_sample_weights* sw, const float** krows, const float** kcols) {
    *krows = sw ? sw->neg_scale_rows : nullptr;
    *kcols = sw ? sw->neg_scale_cols : nullptr;
    if ((*krows == nullptr) != (*kcols == nullptr))
        return fail(CROSSCLR_E_ARG, "neg_scale_rows and neg_scale_cols must be given together");
    return CROSSCLR_OK;
}

// ---- fwd_sums_kernel<T, SW, MODE, ST, SYM>: one descriptor, one launcher ---------------------------------------------------------
// the pass = the kernel's MODE: sums with the common shift, row maxima, sums with per-row shifts; the two score-statistics modes
enum class FwdPass { Sums = 0, RowMax = 1, ShiftedSums = 2, ScoreRows = 3, ScoreDiag = 4 };
struct FwdSums {
    FwdPass pass;
    bool save;                 // ST: leave the exponentials in `stash` (Sums and ShiftedSums only)
    bool symmetric;            // SYM: rows == cols, upper triangle + column partials (ScoreRows: one pass for both directions)
    const void *rows, *cols;
    float* out;
    const float* kcols;        // SW: the columns' negative scales
    const float* shift;        // ShiftedSums: the rows' shifts; score modes: the positive-pair scores
    const float* shift_cols;   // save && ShiftedSums && !symmetric: the columns' shifts, for the transposed records behind the direct ones
    float* stash;              // save: the exponentials; ScoreRows: the active counts
    int* header;               // symmetric: the launch group's header; ScoreRows: the optional hinge mask
    float* colpart;            // symmetric: the column partials
};
// a pass over every tile of rows x cols / over the upper triangle of the local block x against itself
static FwdSums full_pass(FwdPass pass, const void* rows, const void* cols, float* out, const float* kcols, const float* shift) {
    return {pass, false, false, rows, cols, out, kcols, shift, nullptr, nullptr, nullptr, nullptr};
}
static FwdSums symmetric_pass(FwdPass pass, const void* x, const FwdSlot& s, const float* k, const float* shift) {
    return {pass, false, true, x, x, s.out, k, shift, nullptr, nullptr, s.header, s.colpart};
}
static FwdSums saving(FwdSums d, void* stash, const float* shift_cols = nullptr) {
    d.save = true; d.stash = static_cast<float*>(stash); d.shift_cols = shift_cols;
    return d;
}
// crossclr_last_kernel(0): bf16 plans save 2-byte records, the others fp32 fragments; the split-operand instantiations carry <x3_t>
template <typename T> static const char* fwd_sums_label(const FwdSums& d) {
    constexpr bool x3 = std::is_same<T, x3_t>::value;
    if (d.pass == FwdPass::ScoreDiag) return "fwd_sums_kernel (positive-pair scores)";
    if (d.pass == FwdPass::ScoreRows) return "fwd_sums_kernel (score rows)";
    if (d.save && sizeof(T) == 2)
        return d.symmetric ? "fwd_sums_kernel (symmetric, save, bf16 records)"
                           : (d.pass == FwdPass::Sums ? "fwd_sums_kernel (rectangular, save, bf16 records)" : "fwd_sums_kernel (save, bf16 records)");
    if (d.symmetric)
        return d.save ? (x3 ? "fwd_sums_kernel<x3_t> (symmetric, save)" : "fwd_sums_kernel (symmetric, save)")
                      : (x3 ? "fwd_sums_kernel<x3_t> (symmetric)" : "fwd_sums_kernel (symmetric)");
    return d.save ? (x3 ? "fwd_sums_kernel<x3_t> (save)" : "fwd_sums_kernel (save)") : (x3 ? "fwd_sums_kernel<x3_t>" : "fwd_sums_kernel");
}
template <typename T, bool SW, int MODE, bool ST, bool SYM>
static void launch_fwd_sums_as(const crossclr_plan* plan, const Geo& g, const FwdSums& d, void* stream) {
    const int nsplit = MODE == 4 ? 1 : plan->fwd_slots;
    // rows: 128-row blocks; symmetric: one blockIdx.x per PAIR of row blocks (I, ntiles - 1 - I), which walks its tiles without a
    // tiles-per-split; ScoreRows in one pass: the rows of modality 0 against the column tiles of modality 1
    const int row_blocks = SYM ? (MODE == 3 ? plan->bpad / 128 : 2 * plan->bpad / 256) : 2 * plan->bpad / 128;
    const int ntiles = SYM ? (MODE == 3 ? plan->bpad / 128 : 0) : g.col_ranks * 2 * plan->bpad / 128;
    LAUNCH((fwd_sums_kernel<T, SW, MODE, ST, SYM>), dim3(row_blocks, nsplit), dim3(256), stream, (const T*)d.rows, (const T*)d.cols, g,
           (ntiles + nsplit - 1) / nsplit, d.out, d.kcols, d.shift, d.stash, d.header, SYM ? d.colpart : const_cast<float*>(d.shift_cols));
}
// grid, tiles per split and template arguments from the descriptor; only the combinations the kernel's static_asserts allow (and, of the
// score modes, only what the score entry points use: no scales, no split operand) are instantiated
template <typename T>
static int launch_fwd_sums(const crossclr_plan* plan, const Geo& g, const FwdSums& d, void* stream) {
    constexpr bool records = sizeof(T) == 2;      // bf16 plans save bf16 records
    if (d.save && records && d.symmetric && d.pass != FwdPass::Sums)
        return fail(CROSSCLR_E_ARG, "bf16 plans save their exponentials in the single-pass soft-max only");
    if (d.save && records && d.pass != FwdPass::Sums && d.pass != FwdPass::ShiftedSums)
        return fail(CROSSCLR_E_ARG, "bf16 plans save through the generic forward in modes 0 (rectangular) and 2 (two-pass)");
    const bool score = d.pass == FwdPass::ScoreRows || d.pass == FwdPass::ScoreDiag;
    if ((d.save && d.pass != FwdPass::Sums && d.pass != FwdPass::ShiftedSums) || (score && (d.kcols || std::is_same<T, x3_t>::value)))
        return fail(CROSSCLR_E_ARG, "fwd_sums_kernel: no instantiation for pass %d (save %d, scales %d)", (int)d.pass, (int)d.save, d.kcols != nullptr);
    auto soft_max = [&](auto mode, auto st) {      // MODE 0 .. 2: SW x SYM at run time
        constexpr int MODE = decltype(mode)::value;
        constexpr bool ST = decltype(st)::value;
        if (!d.symmetric) {
            if (d.kcols) launch_fwd_sums_as<T, true, MODE, ST, false>(plan, g, d, stream);
            else launch_fwd_sums_as<T, false, MODE, ST, false>(plan, g, d, stream);
        } else if constexpr (!(ST && records && MODE == 2)) {
            if (d.kcols) launch_fwd_sums_as<T, true, MODE, ST, true>(plan, g, d, stream);
            else launch_fwd_sums_as<T, false, MODE, ST, true>(plan, g, d, stream);
        }
    };
    using std::false_type; using std::true_type; using std::integral_constant;
    switch (d.pass) {
        case FwdPass::Sums: if (d.save) soft_max(integral_constant<int, 0>(), true_type()); else soft_max(integral_constant<int, 0>(), false_type()); break;
        case FwdPass::RowMax: soft_max(integral_constant<int, 1>(), false_type()); break;
        case FwdPass::ShiftedSums: if (d.save) soft_max(integral_constant<int, 2>(), true_type()); else soft_max(integral_constant<int, 2>(), false_type()); break;
        case FwdPass::ScoreRows:
            if constexpr (!std::is_same<T, x3_t>::value) {
                if (d.symmetric) launch_fwd_sums_as<T, false, 3, false, true>(plan, g, d, stream);
                else launch_fwd_sums_as<T, false, 3, false, false>(plan, g, d, stream);
            }
            break;
        case FwdPass::ScoreDiag:
            if constexpr (!std::is_same<T, x3_t>::value) launch_fwd_sums_as<T, false, 4, false, false>(plan, g, d, stream);
            break;
    }
    return launch_status(fwd_sums_label<T>(d));
}
// the soft-max passes: the operand type from the plan
static int fwd_sums(const crossclr_plan* plan, const Geo& g, const FwdSums& d, void* stream) {
    return with_plan_type(plan, [&](auto t) { return launch_fwd_sums<typename decltype(t)::type>(plan, g, d, stream); });
}

// the local block evaluated against itself (the single-device case, or the local block of a sharded run): upper triangle + column sums.
// The generic kernels scale the mirrored tiles with the ROWS' array, so their callers also require krows == kcols.
static bool is_local_symmetric_block(const crossclr_plan* plan, const Geo& g, const void* rows, const void* cols) {
    return rows == cols && g.col_ranks == 1 && g.col_rank0 == plan->rank && g.skip_rank < 0 && !env_knobs().disable_symmetric;
}

extern "C" int crossclr_forward(const crossclr_plan* plan, const void* xhat_rows, const void* xhat_cols,
                                int col_ranks, int col_rank0, int skip_rank, float temperature,
                                float negative_weight, float* part, int slot0, void* stream) {
    return crossclr_forward_s(plan, xhat_rows, xhat_cols, col_ranks, col_rank0, skip_rank, temperature, negative_weight, nullptr, nullptr,
                              part, slot0, stream);
}
extern "C" int crossclr_forward_w(const crossclr_plan* plan, const void* xhat_rows, const void* xhat_cols,
                                  int col_ranks, int col_rank0, int skip_rank, float temperature,
                                  float negative_weight, const crossclr_sample_weights* sw, float* part, int slot0,
                                  void* stream) {
    return crossclr_forward_s(plan, xhat_rows, xhat_cols, col_ranks, col_rank0, skip_rank, temperature, negative_weight, sw, nullptr, part,
                              slot0, stream);
}
// shift_rows == NULL: the single-pass soft-max (crossclr_forward_w); else the second pass of the two-pass one, on the generic kernels
extern "C" int crossclr_forward_s(const crossclr_plan* plan, const void* xhat_rows, const void* xhat_cols, int col_ranks,
                                  int col_rank0, int skip_rank, float temperature, float negative_weight,
                                  const crossclr_sample_weights* sw, const float* shift_rows, float* part, int slot0, void* stream) {
    if (!plan || !xhat_rows || !xhat_cols || !part || slot0 < 0) return fail(CROSSCLR_E_ARG, "NULL/negative argument");
    const float *krows, *kcols;
    if (int rk = unpack_k(sw, &krows, &kcols)) return rk;
    Geo g;
    int rc = make_geo(plan, col_ranks, col_rank0, skip_rank, temperature, negative_weight, &g, shift_rows != nullptr);
    if (rc) return rc;
    FwdSlot s;
    if ((rc = fwd_slot(plan, part, slot0, &s))) return rc;
    const bool local = is_local_symmetric_block(plan, g, xhat_rows, xhat_cols);
    const size_t out_bytes = (size_t)plan->fwd_slots * 2 * plan->bpad * sizeof(float);
    if (plan->fast_path && !shift_rows) {
        if (usable_col_ranks(g) <= 0) {
            // nothing to do (every column rank is skipped): leave a dense, all-zero launch behind
            rc = device_zero_header(s.header, stream);
            return rc ? rc : device_zero(s.out, out_bytes, stream);
        }
        rc = fast_forward(plan, g, xhat_rows, xhat_cols, s.out, s.colpart, s.header, local, krows, kcols, stream);
        return rc ? fail(rc, "fast_forward: unsupported Dpad %d", plan->Dpad) : launch_status("fast_fwd_kernel");
    }
    // the second pass marks its launch group dense up front, before the symmetric launch too, and returns early when every column rank is
    // skipped; the single pass on the generic kernels does so only in front of a full launch, which it enqueues even over no columns
    if (shift_rows) {
        if ((rc = device_zero_header(s.header, stream))) return rc;
        if (usable_col_ranks(g) <= 0) return device_zero(s.out, out_bytes, stream);
    }
    const FwdPass pass = shift_rows ? FwdPass::ShiftedSums : FwdPass::Sums;
    if (local && krows == kcols) return fwd_sums(plan, g, symmetric_pass(pass, xhat_rows, s, kcols, shift_rows), stream);
    if (!shift_rows && (rc = device_zero_header(s.header, stream))) return rc;
    return fwd_sums(plan, g, full_pass(pass, xhat_rows, xhat_cols, s.out, kcols, shift_rows), stream);
}

// what the saved backwards of the LOCAL block share: the sample weights (the rows' and the columns' negative scales are one array) and the
// geometry; two_pass: per-row shifts allowed
static int local_saved_args(const crossclr_plan* plan, const crossclr_sample_weights* sw, float temperature, float negative_weight,
                            bool two_pass, const float** k, Geo* g) {
    const float* kcols;
    if (int rk = unpack_k(sw, k, &kcols)) return rk;
    if (*k != kcols) return fail(CROSSCLR_E_ARG, "the local block's row and column negative scales are the same array");
    return make_geo(plan, 1, plan->rank, -1, temperature, negative_weight, g, two_pass);
}
// what the saving forwards of the LOCAL block share beyond local_saved_args: the launch group of the workspace
static int local_save_args(const crossclr_plan* plan, const crossclr_sample_weights* sw, float temperature, float negative_weight, bool two_pass,
                           float* part, int slot0, const float** k, Geo* g, FwdSlot* s) {
    if (int rc = local_saved_args(plan, sw, temperature, negative_weight, two_pass, k, g)) return rc;
    return fwd_slot(plan, part, slot0, s);
}
extern "C" int crossclr_forward_save(const crossclr_plan* plan, const void* xhat, float temperature, float negative_weight,
                                     const crossclr_sample_weights* sw, float* part, int slot0, void* stash, void* stream) {
    if (!plan || !xhat || !part || !stash || slot0 < 0) return fail(CROSSCLR_E_ARG, "NULL/negative argument");
    if (!plan->stash_bytes) return fail(CROSSCLR_E_ARG, "this plan has no save-for-backward path (stash_bytes == 0)");
    const float* k;
    Geo g;
    FwdSlot s;
    int rc = local_save_args(plan, sw, temperature, negative_weight, false, part, slot0, &k, &g, &s);
    if (rc) return rc;
    if (plan->fast_path) {
        rc = fast_forward_save(plan, g, xhat, s.out, s.colpart, s.header, k, stash, stream);
        return rc ? fail(rc, "fast_forward_save: unsupported Dpad %d", plan->Dpad) : launch_status("fast_fwd_kernel (save)");
    }
    // wide bf16 plans: upper triangle, bf16 records in the register-resident layout; exact-fp32 mode (and BF16X3: the same launch on the
    // split operand): upper triangle, every fragment stored twice (as evaluated + transposed)
    if (plan->mode == CROSSCLR_MODE_BF16 || !env_knobs().disable_symmetric)
        return fwd_sums(plan, g, saving(symmetric_pass(FwdPass::Sums, xhat, s, k, nullptr), stash), stream);
    if ((rc = device_zero_header(s.header, stream))) return rc;
    return fwd_sums(plan, g, saving(full_pass(FwdPass::Sums, xhat, xhat, s.out, k, nullptr), stash), stream);
}

// bwd_saved32_kernel / bwd_saved_x3_kernel (crossclr_kernels_saved32.h): DC = 256, 128 or 64 columns of D per thread block (with_d_chunk)
// and `ntiles` 32-column tiles cut into plan->bwd_slices slices WITHOUT the even rounding of fast_backward_saved
static dim3 saved32_grid(const crossclr_plan* plan, int DC) { return dim3(2 * plan->bpad / 64, plan->Dpad / DC, (unsigned)plan->bwd_slices); }
static int saved32_tps(const crossclr_plan* plan, int ntiles) { return (ntiles + plan->bwd_slices - 1) / plan->bwd_slices; }

// BF16X3 plans: the saved backward on the split operand, single pass (RM = false) or two-pass (RM = true)
template <bool RM>
static int backward_saved_x3(const crossclr_plan* plan, const Geo& g, const void* xhat, const void* stash, const float* rz, const float* wrz,
                             const float* k, float* gbuf, int accumulate, void* stream) {
    const int tps = saved32_tps(plan, 2 * plan->bpad / 32);
    with_d_chunk<256, 128, 64>(plan->Dpad, [&](auto dc) {
        constexpr int DC = decltype(dc)::value;
        if (k) LAUNCH((bwd_saved_x3_kernel<DC, true, RM>), saved32_grid(plan, DC), dim3(256), stream, (const x3_t*)xhat, (const float*)stash, g, rz,
                      wrz, gbuf, accumulate, tps, k);
        else LAUNCH((bwd_saved_x3_kernel<DC, false, RM>), saved32_grid(plan, DC), dim3(256), stream, (const x3_t*)xhat, (const float*)stash, g, rz,
                    wrz, gbuf, accumulate, tps, k);
    });
    return launch_status(RM ? "bwd_saved_x3_kernel (two-pass)" : "bwd_saved_x3_kernel");
}
// exact-fp32 plans: the saved backward over `ntiles` column tiles -- the local block (rzc / wrzc / kc unused) or, RECT, this rank's rows
// against the gathered operand x with the gathered column statistics; single pass or two-pass (RM)
template <bool RM, bool RECT>
static int launch_saved32(const crossclr_plan* plan, const Geo& g, const void* x, const void* stash, const float* rz, const float* wrz,
                          const float* rzc, const float* wrzc, const float* k, const float* kc, int ntiles, float* gbuf, int accumulate,
                          void* stream) {
    const int tps = saved32_tps(plan, ntiles);
    with_d_chunk<256, 128, 64>(plan->Dpad, [&](auto dc) {
        constexpr int DC = decltype(dc)::value;
        if (k) LAUNCH((bwd_saved32_kernel<DC, true, RM, RECT>), saved32_grid(plan, DC), dim3(256), stream, (const float*)x, (const float*)stash, g,
                      rz, wrz, gbuf, accumulate, tps, k, rzc, wrzc, kc);
        else LAUNCH((bwd_saved32_kernel<DC, false, RM, RECT>), saved32_grid(plan, DC), dim3(256), stream, (const float*)x, (const float*)stash, g,
                    rz, wrz, gbuf, accumulate, tps, k, rzc, wrzc, kc);
    });
    return launch_status(RECT ? (RM ? "bwd_saved32_kernel (rect, two-pass)" : "bwd_saved32_kernel (rect)")
                              : (RM ? "bwd_saved32_kernel (two-pass)" : "bwd_saved32_kernel"));
}

// The two-pass regime's W = U rz_p + Ut rz_q as two launches of the bf16 saved backward: the rows' side weighs with the ROW statistics only
// (columns' side: zeros), the columns' side with the COLUMN statistics only (rows' side: zeros) and accumulates
struct SavedSide { SavedBlock block; const Geo& g; const void* stash; const char* what; };
static int saved_two_pass(const crossclr_plan* plan, const void* x, const SavedSide& rows, const SavedSide& cols, const float* zeros,
                          const float* rz_rows, const float* wrz_rows, const float* rz_cols, const float* wrz_cols, const float* krows,
                          const float* kcols, float* gbuf, int accumulate, const char* label, void* stream) {
    int rc = fast_backward_saved({rows.block, SavedOperand::RowMajor}, plan, rows.g, x, rows.stash, rz_rows, wrz_rows, zeros, zeros, gbuf,
                                 accumulate, krows, kcols, stream);
    if (rc) return fail(rc, "fast_backward_saved (%s): unsupported Dpad %d", rows.what, plan->Dpad);
    rc = fast_backward_saved({cols.block, SavedOperand::RowMajor}, plan, cols.g, x, cols.stash, zeros, zeros, rz_cols, wrz_cols, gbuf, 1, krows,
                             kcols, stream);
    return rc ? fail(rc, "fast_backward_saved (%s): unsupported Dpad %d", cols.what, plan->Dpad) : launch_status(label);
}
// the Geo of a SavedBlock::RectTransposed launch: `segments` rank segments per row of the rectangular stash, the output rows (rank `row_rank`)
// at segment `which` of it, the columns = this rank's own rows
static Geo transposed_geo(const crossclr_plan* plan, Geo g, int segments, int which, int row_rank) {
    g.col_ranks = segments; g.skip_rank = which; g.col_rank0 = plan->rank; g.col_wrap = 0; g.row_rank = row_rank;
    return g;
}

// crossclr_backward_saved (RowMajor), _saved_xf (FragmentOne) and _saved_xfp (FragmentPair); fn: the entry point's name, for its refusals
static int backward_saved_local(const char* fn, SavedOperand operand, const crossclr_plan* plan, const void* x, const void* stash,
                                float temperature, float negative_weight, const float* rz, const float* wrz,
                                const crossclr_sample_weights* sw, float* gbuf, int accumulate, void* stream) {
    if (!plan || !x || !stash || !rz || !wrz || !gbuf) return fail(CROSSCLR_E_ARG, "NULL argument");
    const bool row_major = operand == SavedOperand::RowMajor, pair = operand == SavedOperand::FragmentPair;
    if (row_major && !plan->stash_bytes) return fail(CROSSCLR_E_ARG, "this plan has no save-for-backward path (stash_bytes == 0)");
    if (!row_major && (!plan->stash_bytes || !plan->xf_bytes))
        return fail(CROSSCLR_E_ARG, "this plan has no fragment-major saved backward (stash_bytes / xf_bytes == 0)");
    if (pair && plan->stash_bytes >= ((size_t)1 << 32))
        return fail(CROSSCLR_E_ARG, "%s addresses the saved exponentials with 32-bit offsets (stash of %zu bytes): use crossclr_backward_saved_xf", fn, plan->stash_bytes);
    const float* k;
    Geo g;
    int rc = local_saved_args(plan, sw, temperature, negative_weight, false, &k, &g);
    if (rc) return rc;
    if (row_major && is_x3(plan)) return backward_saved_x3<false>(plan, g, x, stash, rz, wrz, k, gbuf, accumulate, stream);
    if (row_major && !plan->fast_path && plan->mode == CROSSCLR_MODE_FP32)   // exact-fp32 mode
        return launch_saved32<false, false>(plan, g, x, stash, rz, wrz, kNoF, kNoF, k, kNoF, 2 * plan->bpad / 32, gbuf, accumulate, stream);
    rc = fast_backward_saved({SavedBlock::Local, operand}, plan, g, x, stash, rz, wrz, rz, wrz, gbuf, accumulate, k, k, stream);
    if (rc) return fail(rc, "fast_backward_saved%s: unsupported Dpad %d", row_major ? "" : (pair ? " (xfp)" : " (xf)"), plan->Dpad);
    return launch_status(row_major ? "fast_bwd_dsl_kernel" : (pair ? "fast_bwd_xfp_kernel" : "fast_bwd_dsl_kernel (xf)"));
}
extern "C" int crossclr_backward_saved(const crossclr_plan* plan, const void* xhat, const void* stash, float temperature,
                                       float negative_weight, const float* rz, const float* wrz,
                                       const crossclr_sample_weights* sw, float* gbuf, int accumulate, void* stream) {
    return backward_saved_local("crossclr_backward_saved", SavedOperand::RowMajor, plan, xhat, stash, temperature, negative_weight, rz, wrz, sw,
                                gbuf, accumulate, stream);
}
extern "C" int crossclr_backward_saved_xf(const crossclr_plan* plan, const void* xhat_xf, const void* stash, float temperature,
                                          float negative_weight, const float* rz, const float* wrz,
                                          const crossclr_sample_weights* sw, float* gbuf, int accumulate, void* stream) {
    return backward_saved_local("crossclr_backward_saved_xf", SavedOperand::FragmentOne, plan, xhat_xf, stash, temperature, negative_weight, rz,
                                wrz, sw, gbuf, accumulate, stream);
}
extern "C" int crossclr_backward_saved_xfp(const crossclr_plan* plan, const void* xhat_xf, const void* stash, float temperature,
                                           float negative_weight, const float* rz, const float* wrz,
                                           const crossclr_sample_weights* sw, float* gbuf, int accumulate, void* stream) {
    return backward_saved_local("crossclr_backward_saved_xfp", SavedOperand::FragmentPair, plan, xhat_xf, stash, temperature, negative_weight, rz,
                                wrz, sw, gbuf, accumulate, stream);
}

extern "C" int crossclr_forward_pairs(const crossclr_plan* plan, const void* xhat_rows, const void* xhat_all, int first_rank,
                                      int nranks, float temperature, float negative_weight,
                                      const crossclr_sample_weights* sw, float* part, int slot0, float* colsum_out,
                                      void* stream) {
    if (!plan || !xhat_rows || !xhat_all || !part || !colsum_out) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (!plan->fast_path) return fail(CROSSCLR_E_ARG, "crossclr_forward_pairs needs the register-resident bf16 path");
    if (first_rank < 0 || first_rank >= plan->world || nranks < 1 || nranks > (plan->world - 1) / 2)
        return fail(CROSSCLR_E_ARG, "bad first_rank/nranks %d/%d for world %d", first_rank, nranks, plan->world);
    FwdSlot s;
    if (int rs = fwd_slot(plan, part, slot0, &s)) return rs;
    for (int i = 0; i < nranks; ++i)
        if ((first_rank + i) % plan->world == plan->rank) return fail(CROSSCLR_E_ARG, "the pair range must not contain this rank");
    const float *krows, *kcols;
    if (int rk = unpack_k(sw, &krows, &kcols)) return rk;
    Geo g;
    int rc = make_geo(plan, nranks, first_rank, -1, temperature, negative_weight, &g);
    if (rc) return rc;
    g.col_wrap = plan->world;
    rc = fast_forward(plan, g, xhat_rows, xhat_all, s.out, s.paircol, s.header, false, krows, kcols, stream, true);
    if (rc) return fail(rc, "fast_forward: unsupported Dpad %d", plan->Dpad);
    const int nrb = 2 * plan->bpad / (32 * fast_fwd_tpr(plan->Dpad));
    const int ncols = nranks * 2 * plan->bpad;
    LAUNCH(colsum_reduce_kernel, dim3((ncols + 255) / 256), dim3(256), stream, (const float*)s.paircol, nrb, ncols, colsum_out);
    return launch_status("fast_fwd_kernel (pairs)");
}

extern "C" int crossclr_forward_add(const crossclr_plan* plan, float* part, int slot0, const float* vec, void* stream) {
    if (!plan || !part) return fail(CROSSCLR_E_ARG, "NULL argument");
    FwdSlot s;
    if (int rc = fwd_slot(plan, part, slot0, &s)) return rc;
    const int n = 2 * plan->bpad;
    LAUNCH(fwd_add_kernel, dim3((n + 255) / 256), dim3(256), stream, vec, n, s.out, s.header);
    return launch_status("fwd_add_kernel");
}

// ticket != NULL (crossclr_step_forward; an int the step's first kernel has cleared): the finish kernel's last block forms the sum -- one launch
static int forward_finish_impl(const crossclr_plan* plan, const float* part, int nslots,
                               const float* diag_cos, float temperature, float negative_weight,
                               const crossclr_sample_weights* sw, const float* shift_rows, float* logz, float* rz,
                               float* wrz, double* loss_sum, void* stream, int* ticket) {
    if (!plan || !part || !diag_cos || !logz || !rz || !wrz || !loss_sum || plan->fwd_slots <= 0 || nslots <= 0 ||
        nslots % plan->fwd_slots != 0 || nslots / plan->fwd_slots > kLaunchGroups)
        return fail(CROSSCLR_E_ARG, "NULL argument / nslots must be fwd_slots times the number of launch groups (1..%d)", kLaunchGroups);
    Geo g;
    int rc = make_geo(plan, 1, plan->rank, -1, temperature, negative_weight, &g, shift_rows != nullptr);
    if (rc) return rc;
    if ((g.row_shift != 0) != (shift_rows != nullptr))
        return fail(CROSSCLR_E_ARG, "shift_rows must be given exactly when crossclr_needs_row_shift(temperature, negative_weight)");
    const int nb = plan->loss_ws_doubles - 1;
    const int nlaunch = nslots / plan->fwd_slots;
    LAUNCH(fwd_finish_kernel, dim3(nb), dim3(256), stream, part, nlaunch, plan->fwd_slots, g, diag_cos, 1.0f / temperature,
           negative_weight, logz, rz, wrz, loss_sum, part + ws_colpart_off(plan),
           reinterpret_cast<const int*>(part + ws_flag_off(plan)), sw ? sw->neg_scale_rows : nullptr,
           sw ? sw->loss_weight : nullptr, shift_rows, ticket, 1.0 / (2.0 * (double)plan->b * (double)plan->world));
    if (!ticket) LAUNCH(fwd_finish_reduce_kernel, dim3(1), dim3(64), stream, loss_sum, nb, 1.0 / (2.0 * (double)plan->b * (double)plan->world));
    return launch_status("fwd_finish_kernel");
}
extern "C" int crossclr_forward_finish(const crossclr_plan* plan, const float* part, int nslots,
                                       const float* diag_cos, float temperature, float negative_weight,
                                       float* logz, float* rz, float* wrz, double* loss_sum, void* stream) {
    return forward_finish_impl(plan, part, nslots, diag_cos, temperature, negative_weight, nullptr, nullptr, logz, rz, wrz, loss_sum, stream, nullptr);
}
extern "C" int crossclr_forward_finish_w(const crossclr_plan* plan, const float* part, int nslots,
                                         const float* diag_cos, float temperature, float negative_weight,
                                         const crossclr_sample_weights* sw, float* logz, float* rz, float* wrz,
                                         double* loss_sum, void* stream) {
    return forward_finish_impl(plan, part, nslots, diag_cos, temperature, negative_weight, sw, nullptr, logz, rz, wrz, loss_sum, stream, nullptr);
}
extern "C" int crossclr_forward_finish_s(const crossclr_plan* plan, const float* part, int nslots,
                                         const float* diag_cos, float temperature, float negative_weight,
                                         const crossclr_sample_weights* sw, const float* shift_rows, float* logz, float* rz,
                                         float* wrz, double* loss_sum, void* stream) {
    return forward_finish_impl(plan, part, nslots, diag_cos, temperature, negative_weight, sw, shift_rows, logz, rz, wrz, loss_sum, stream, nullptr);
}

// ---- two-pass soft-max for small temperatures (max |logit| > 128) ------------------------------------------------------
extern "C" int crossclr_needs_row_shift(float temperature, float negative_weight) {
    return (temperature > 0.f && isfinite(temperature) && isfinite(negative_weight) && needs_row_shift(temperature, negative_weight)) ? 1 : 0;
}

extern "C" int crossclr_forward_rowmax(const crossclr_plan* plan, const void* xhat_rows, const void* xhat_cols, int col_ranks,
                                       int col_rank0, int skip_rank, float temperature, float negative_weight,
                                       const crossclr_sample_weights* sw, float* part, float* shift_rows, int accumulate,
                                       void* stream) {
    if (!plan || !xhat_rows || !xhat_cols || !part || !shift_rows) return fail(CROSSCLR_E_ARG, "NULL argument");
    const float *krows, *kcols;
    if (int rk = unpack_k(sw, &krows, &kcols)) return rk;
    Geo g;
    int rc = make_geo(plan, col_ranks, col_rank0, skip_rank, temperature, negative_weight, &g, true);
    if (rc) return rc;
    const int n = 2 * plan->bpad;
    int nslots = plan->fwd_slots;
    const float* colpart = nullptr;
    if (usable_col_ranks(g) <= 0) nslots = 0;   // nothing to look at: only the self pair / the previous value
    else if (is_local_symmetric_block(plan, g, xhat_rows, xhat_cols) && krows == kcols) {   // upper triangle, column maxima for the mirrored tiles
        const FwdSlot s = fwd_group(plan, part, 0);   // (launch group 0 and its header: rewritten by the pass that follows)
        if ((rc = fwd_sums(plan, g, symmetric_pass(FwdPass::RowMax, xhat_rows, s, kcols, nullptr), stream))) return rc;
        colpart = s.colpart;
    } else if ((rc = fwd_sums(plan, g, full_pass(FwdPass::RowMax, xhat_rows, xhat_cols, part, kcols, nullptr), stream))) return rc;
    LAUNCH(rowmax_combine_kernel, dim3((n + 255) / 256), dim3(256), stream, (const float*)part, nslots, n, krows, accumulate, shift_rows, colpart);
    return launch_status("rowmax_combine_kernel");
}

// the two-pass regime's save-for-backward pair (exact-fp32 plans, local block): U and Ut, twice the single-pass stash
// bf16 register-resident plans in the two-pass regime: the FULL matrix of bf16 records U[p][q] = exp2(x - shift[p]) in the rectangular layout
// of a one-rank remote block, followed by 2 bpad floats of zeros (crossclr_backward_saved_s passes them as the statistics of the side a
// launch must not weigh: W = U rz_p + U^T rz_q is formed as two launches of the saved backward, direct and transposed)
static size_t rect_bytes_s(const crossclr_plan* plan) {
    if (!plan || plan->mode != CROSSCLR_MODE_BF16 || !plan->stash_bytes) return 0;
    if (plan->fast_path) return fast_stash_bytes_rect(plan->bpad, plan->Dpad, 1);
    return plan->Dpad > 1024 ? wide_stash_bytes_rect(plan->bpad, 1) : 0;      // wide plans: the generic second pass writes U AND Ut (below)
}
// wide bf16 plans (Dpad > 1024) have no transposed launch of the saved backward: their second pass writes Ut behind U (like a remote block's)
// and the backward is two DIRECT launches, over U with the rows' statistics and over Ut with the columns'
static bool wide_two_pass(const crossclr_plan* plan) { return plan && plan->mode == CROSSCLR_MODE_BF16 && !plan->fast_path && plan->Dpad > 1024; }
static size_t stash_bytes_s(const crossclr_plan* plan) {
    if (!plan || !plan->stash_bytes) return 0;
    if (plan->mode == CROSSCLR_MODE_BF16) {
        const size_t rb = rect_bytes_s(plan);
        return rb ? (wide_two_pass(plan) ? 2 : 1) * rb + (size_t)2 * plan->bpad * 4 : 0;
    }
    if (plan->fast_path || (plan->mode != CROSSCLR_MODE_FP32 && plan->mode != CROSSCLR_MODE_BF16X3)) return 0;
    return 2 * plan->stash_bytes <= ((size_t)16 << 30) ? 2 * plan->stash_bytes : 0;
}
extern "C" size_t crossclr_stash_bytes_s(const crossclr_plan* plan) { return stash_bytes_s(plan); }

extern "C" int crossclr_forward_save_s(const crossclr_plan* plan, const void* xhat, float temperature, float negative_weight,
                                       const crossclr_sample_weights* sw, const float* shift, float* part, int slot0, void* stash,
                                       void* stream) {
    if (!plan || !xhat || !shift || !part || !stash || slot0 < 0) return fail(CROSSCLR_E_ARG, "NULL/negative argument");
    if (!stash_bytes_s(plan)) return fail(CROSSCLR_E_ARG, "this plan has no two-pass save-for-backward path (crossclr_stash_bytes_s == 0)");
    const float* k;
    Geo g;
    FwdSlot s;
    int rc = local_save_args(plan, sw, temperature, negative_weight, true, part, slot0, &k, &g, &s);
    if (rc) return rc;
    const bool records = plan->mode == CROSSCLR_MODE_BF16;   // full (non-symmetric) second pass: bf16 records + the zero statistics behind them
    if (!records && !env_knobs().disable_symmetric)
        return fwd_sums(plan, g, saving(symmetric_pass(FwdPass::ShiftedSums, xhat, s, k, shift), stash), stream);
    if ((rc = device_zero_header(s.header, stream))) return rc;
    if (records) {
        rc = device_zero(static_cast<unsigned char*>(stash) + (wide_two_pass(plan) ? 2 : 1) * rect_bytes_s(plan), (size_t)2 * plan->bpad * 4, stream);
        if (rc) return rc;
    }
    return fwd_sums(plan, g, saving(full_pass(FwdPass::ShiftedSums, xhat, xhat, s.out, k, shift), stash, wide_two_pass(plan) ? shift : nullptr), stream);
}

extern "C" int crossclr_backward_saved_s(const crossclr_plan* plan, const void* xhat, const void* stash, float temperature,
                                         float negative_weight, const float* rz, const float* wrz,
                                         const crossclr_sample_weights* sw, float* gbuf, int accumulate, void* stream) {
    if (!plan || !xhat || !stash || !rz || !wrz || !gbuf) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (!stash_bytes_s(plan)) return fail(CROSSCLR_E_ARG, "this plan has no two-pass save-for-backward path (crossclr_stash_bytes_s == 0)");
    const float* k;
    Geo g;
    int rc = local_saved_args(plan, sw, temperature, negative_weight, true, &k, &g);
    if (rc) return rc;
    if (plan->mode == CROSSCLR_MODE_BF16) {
        // W[p][q] = U[p][q] rz_p + U[q][p] rz_q as two 8 B^2 D launches of the saved backward (saved_two_pass) instead of the
        // 16 B^2 D (1 + ...) recompute of the generic kernel
        const unsigned char* U = static_cast<const unsigned char*>(stash);
        const size_t rb = rect_bytes_s(plan);
        if (wide_two_pass(plan))     // U rz_p from the first array, Ut rz_q from the second: two direct launches of the D-slice kernel in column parts
            return saved_two_pass(plan, xhat, {SavedBlock::Rect, g, U, "two-pass, wide, rows' side"},
                                  {SavedBlock::Rect, g, U + rb, "two-pass, wide, columns' side"}, reinterpret_cast<const float*>(U + 2 * rb), rz,
                                  wrz, rz, wrz, k, k, gbuf, accumulate, "fast_bwd_dsl_kernel (two-pass pair, wide)", stream);
        // one array: the direct launch, then the transposed one with the statistics of the rows it contracts over
        return saved_two_pass(plan, xhat, {SavedBlock::Rect, g, U, "two-pass, direct"},
                              {SavedBlock::RectTransposed, transposed_geo(plan, g, 1, 0, plan->rank), U, "two-pass, transposed"},
                              reinterpret_cast<const float*>(U + rb), rz, wrz, rz, wrz, k, k, gbuf, accumulate,
                              "fast_bwd_dsl_kernel (two-pass pair)", stream);
    }
    if (is_x3(plan)) return backward_saved_x3<true>(plan, g, xhat, stash, rz, wrz, k, gbuf, accumulate, stream);
    return launch_saved32<true, false>(plan, g, xhat, stash, rz, wrz, kNoF, kNoF, k, kNoF, 2 * plan->bpad / 32, gbuf, accumulate, stream);
}

// ------------------------------------------------------------------------------------------------
// the generic gradient kernels' grid: 64-row blocks x DC-column chunks of D x plan->bwd_slices column slices
static dim3 bwd_grid(const crossclr_plan* p, int DC) { return dim3(2 * p->bpad / 64, p->Dpad / DC, (unsigned)p->bwd_slices); }
template <typename T>
static int backward_generic(const crossclr_plan* p, const Geo& g, const void* rows, const void* cols,
                            const float* rz_rows, const float* wrz_rows, const float* rz_cols,
                            const float* wrz_cols, float* gbuf, int accumulate, const float* krows, const float* kcols,
                            const float* shift_rows, const float* shift_cols, void* stream) {
    const int tps = (usable_col_ranks(g) * 2 * p->bpad / 64 + p->bwd_slices - 1) / p->bwd_slices;   // usable column tiles per slice
    // the generic backward slices D by DC and gbuf by plan->bwd_slices column slices; a plan made for the register-resident
    // kernels has the slice count of THEIR tiling, which is a valid (just not tuned) slice count here too
    with_d_chunk<512, 256, 128, 64>(p->Dpad, [&](auto dc) {
        constexpr int DC = decltype(dc)::value;
        auto launch = [&](auto sw, auto rm) {
            LAUNCH((bwd_kernel<T, DC, decltype(sw)::value, decltype(rm)::value>), bwd_grid(p, DC), dim3(256), stream, (const T*)rows, (const T*)cols,
                   g, rz_rows, wrz_rows, rz_cols, wrz_cols, gbuf, accumulate, tps, krows, kcols, shift_rows, shift_cols);
        };
        if (shift_rows) { if (krows) launch(std::true_type(), std::true_type()); else launch(std::false_type(), std::true_type()); }
        else { if (krows) launch(std::true_type(), std::false_type()); else launch(std::false_type(), std::false_type()); }
    });
    return launch_status(glabel<T>("bwd_kernel", "bwd_kernel<x3_t>"));
}

extern "C" int crossclr_backward(const crossclr_plan* plan, const void* xhat_rows, const void* xhat_cols,
                                 int col_ranks, int col_rank0, int skip_rank, float temperature,
                                 float negative_weight, const float* rz_rows, const float* wrz_rows,
                                 const float* rz_cols, const float* wrz_cols, float* gbuf, int accumulate,
                                 void* stream) {
    return crossclr_backward_s(plan, xhat_rows, xhat_cols, col_ranks, col_rank0, skip_rank, temperature, negative_weight, rz_rows, wrz_rows,
                               rz_cols, wrz_cols, nullptr, nullptr, nullptr, gbuf, accumulate, stream);
}
extern "C" int crossclr_backward_w(const crossclr_plan* plan, const void* xhat_rows, const void* xhat_cols,
                                   int col_ranks, int col_rank0, int skip_rank, float temperature,
                                   float negative_weight, const float* rz_rows, const float* wrz_rows,
                                   const float* rz_cols, const float* wrz_cols, const crossclr_sample_weights* sw,
                                   float* gbuf, int accumulate, void* stream) {
    return crossclr_backward_s(plan, xhat_rows, xhat_cols, col_ranks, col_rank0, skip_rank, temperature, negative_weight, rz_rows, wrz_rows,
                               rz_cols, wrz_cols, sw, nullptr, nullptr, gbuf, accumulate, stream);
}
// no shifts: the single-pass soft-max (crossclr_backward_w); both: the two-pass one, on the generic kernel
extern "C" int crossclr_backward_s(const crossclr_plan* plan, const void* xhat_rows, const void* xhat_cols, int col_ranks,
                                   int col_rank0, int skip_rank, float temperature, float negative_weight,
                                   const float* rz_rows, const float* wrz_rows, const float* rz_cols, const float* wrz_cols,
                                   const crossclr_sample_weights* sw, const float* shift_rows, const float* shift_cols,
                                   float* gbuf, int accumulate, void* stream) {
    const bool two_pass = shift_rows || shift_cols;
    if (!plan || !xhat_rows || !xhat_cols || !rz_rows || !wrz_rows || !rz_cols || !wrz_cols || !gbuf || (two_pass && (!shift_rows || !shift_cols)))
        return fail(CROSSCLR_E_ARG, "NULL argument");
    const float *krows, *kcols;
    if (int rk = unpack_k(sw, &krows, &kcols)) return rk;
    Geo g;
    int rc = make_geo(plan, col_ranks, col_rank0, skip_rank, temperature, negative_weight, &g, two_pass);
    if (rc) return rc;
    if (plan->fast_bwd && !two_pass) {
        rc = plan->fast_bwd == 2
                 ? fast_backward16(plan, g, xhat_rows, xhat_cols, rz_rows, wrz_rows, rz_cols, wrz_cols, gbuf, accumulate, krows, kcols, stream)
                 : fast_backward(plan, g, xhat_rows, xhat_cols, rz_rows, wrz_rows, rz_cols, wrz_cols, gbuf, accumulate, krows, kcols, stream);
        return rc ? fail(rc, "fast backward: unsupported Dpad %d", plan->Dpad) : launch_status("fast_bwd_kernel");
    }
    return with_plan_type(plan, [&](auto t) {
        return backward_generic<typename decltype(t)::type>(plan, g, xhat_rows, xhat_cols, rz_rows, wrz_rows, rz_cols, wrz_cols, gbuf, accumulate,
                                                            krows, kcols, shift_rows, shift_cols, stream);
    });
}

// ---- rectangular blocks of the sharded step with saved exponentials ------------------------------------------------------
// `first_rank`, `nranks`: column ranks first_rank .. first_rank+nranks-1 (mod plan->world) of the WHOLE gathered operand.
static int rect_geo(const crossclr_plan* plan, int first_rank, int nranks, float temperature, float negative_weight, Geo* g,
                    bool allow_row_shift = false) {
    if (is_x3(plan)) return refuse_x3("rank-range entry points");
    if (first_rank < 0 || first_rank >= plan->world || nranks < 1 || nranks >= plan->world)
        return fail(CROSSCLR_E_ARG, "bad first_rank/nranks %d/%d for world %d", first_rank, nranks, plan->world);
    for (int i = 0; i < nranks; ++i)
        if ((first_rank + i) % plan->world == plan->rank) return fail(CROSSCLR_E_ARG, "the rank range must not contain this rank");
    int rc = make_geo(plan, nranks, first_rank, -1, temperature, negative_weight, g, allow_row_shift);
    if (rc) return rc;
    g->col_wrap = plan->world;
    return CROSSCLR_OK;
}

extern "C" size_t crossclr_rect_stash_bytes(const crossclr_plan* plan, int nranks) {
    if (!plan || !plan->stash_bytes || nranks < 1) return 0;
    if (!plan->fast_path && plan->mode == CROSSCLR_MODE_FP32) {   // exact-fp32 plans: fp32 fragments of the rectangular block, up to 16 GiB
        const size_t sb = (size_t)(2 * plan->bpad / 32) * (size_t)(2 * plan->bpad / 32) * (size_t)nranks * 4096;
        return sb <= ((size_t)16 << 30) && plan->operand_bytes * (size_t)plan->world < ((size_t)1 << 32) ? sb : 0;
    }
    if (!plan->fast_path && plan->mode == CROSSCLR_MODE_BF16 && plan->Dpad > 1024)   // wide bf16 plans: bf16 records of the generic forward
        return plan->operand_bytes * (size_t)plan->world < ((size_t)1 << 32) ? wide_stash_bytes_rect(plan->bpad, nranks) : 0;
    if (!plan->fast_path) return 0;
    return fast_stash_bytes_rect(plan->bpad, plan->Dpad, nranks);
}

extern "C" int crossclr_forward_rect_save(const crossclr_plan* plan, const void* xhat_rows, const void* xhat_all, int first_rank,
                                          int nranks, int with_colsums, float temperature, float negative_weight,
                                          const crossclr_sample_weights* sw, float* part, int slot0, float* colsum_out,
                                          void* stash, void* stream) {
    if (!plan || !xhat_rows || !xhat_all || !part || !stash || (with_colsums && !colsum_out)) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (is_x3(plan)) return refuse_x3("crossclr_forward_rect_save");
    if (plan->stash_bytes && !plan->fast_path && (plan->mode == CROSSCLR_MODE_FP32 || plan->Dpad > 1024)) {
        // exact-fp32 plans: the generic forward over the rank range, leaving its fp32 fragments behind ([row group][fragments of the range]);
        // wide bf16 plans (Dpad > 1024): the same launch leaves bf16 records ([row group][tile of the range]: fast_bwd_dsl_kernel<..., MODE 1>)
        if (with_colsums) return fail(CROSSCLR_E_ARG, "plans on the generic forward have no pair scheme (with_colsums must be 0)");
        if (!crossclr_rect_stash_bytes(plan, nranks)) return fail(CROSSCLR_E_ARG, "rectangular stash too large for this plan");
        FwdSlot s32;
        if (int rs = fwd_slot(plan, part, slot0, &s32)) return rs;
        const float *kr32, *kc32;
        if (int rk = unpack_k(sw, &kr32, &kc32)) return rk;
        Geo g32;
        int rc32 = rect_geo(plan, first_rank, nranks, temperature, negative_weight, &g32);
        if (rc32) return rc32;
        if ((rc32 = device_zero_header(s32.header, stream))) return rc32;
        return fwd_sums(plan, g32, saving(full_pass(FwdPass::Sums, xhat_rows, xhat_all, s32.out, kc32, nullptr), stash), stream);
    }
    if (!plan->stash_bytes || !plan->fast_path) return fail(CROSSCLR_E_ARG, "this plan has no save-for-backward path for remote blocks");
    if (with_colsums && nranks > (plan->world - 1) / 2) return fail(CROSSCLR_E_ARG, "a pair range holds at most (world-1)/2 ranks");
    FwdSlot s;
    if (int rs = fwd_slot(plan, part, slot0, &s)) return rs;
    const float *krows, *kcols;
    if (int rk = unpack_k(sw, &krows, &kcols)) return rk;
    Geo g;
    int rc = rect_geo(plan, first_rank, nranks, temperature, negative_weight, &g);
    if (rc) return rc;
    const FwdWork wk = fast_forward_work(plan, nranks, -1, false, with_colsums != 0);
    rc = fast_forward_pipe(plan, g, wk, xhat_rows, xhat_all, s.out, s.paircol, s.header, with_colsums ? 3 : 2, krows, kcols, stash, stream);
    if (rc) return fail(rc, "fast_forward_pipe: unsupported Dpad %d", plan->Dpad);
    if (with_colsums) {
        const int nrb = 2 * plan->bpad / (32 * fast_fwd_tpr(plan->Dpad));
        const int ncols = nranks * 2 * plan->bpad;
        LAUNCH(colsum_reduce_kernel, dim3((ncols + 255) / 256), dim3(256), stream, (const float*)s.paircol, nrb, ncols, colsum_out);
    }
    return launch_status("fast_fwd_pipe_kernel (rect, save)");
}

// what the saved backwards of a rectangular block share: the sample weights and the geometry of the rank range
static int rect_saved_args(const crossclr_plan* plan, const crossclr_sample_weights* sw, int first_rank, int nranks, float temperature,
                           float negative_weight, bool two_pass, const float** krows, const float** kcols, Geo* g) {
    if (int rk = unpack_k(sw, krows, kcols)) return rk;
    return rect_geo(plan, first_rank, nranks, temperature, negative_weight, g, two_pass);
}

extern "C" int crossclr_backward_rect_saved(const crossclr_plan* plan, const void* xhat_all, const void* stash, int first_rank,
                                            int nranks, float temperature, float negative_weight, const float* rz_rows,
                                            const float* wrz_rows, const float* rz_all, const float* wrz_all,
                                            const crossclr_sample_weights* sw, float* gbuf, int accumulate, void* stream) {
    if (!plan || !xhat_all || !stash || !rz_rows || !wrz_rows || !rz_all || !wrz_all || !gbuf) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (is_x3(plan)) return refuse_x3("crossclr_backward_rect_saved");
    const bool exact = plan->stash_bytes && !plan->fast_path && plan->mode == CROSSCLR_MODE_FP32;   // exact-fp32 plans: bwd_saved32_kernel<..., RECT>
    if (!exact && (!plan->stash_bytes || !(plan->fast_path || (plan->mode == CROSSCLR_MODE_BF16 && plan->Dpad > 1024))))
        return fail(CROSSCLR_E_ARG, "this plan has no save-for-backward path for remote blocks");
    const float *krows, *kcols;
    Geo g;
    int rc = rect_saved_args(plan, sw, first_rank, nranks, temperature, negative_weight, false, &krows, &kcols, &g);
    if (rc) return rc;
    if (exact)
        return launch_saved32<false, true>(plan, g, xhat_all, stash, rz_rows, wrz_rows, rz_all, wrz_all, krows, kcols,
                                           nranks * (2 * plan->bpad / 32), gbuf, accumulate, stream);
    rc = fast_backward_saved({SavedBlock::Rect, SavedOperand::RowMajor}, plan, g, xhat_all, stash, rz_rows, wrz_rows, rz_all, wrz_all, gbuf,
                             accumulate, krows, kcols, stream);
    return rc ? fail(rc, "fast_backward_saved: unsupported Dpad %d", plan->Dpad) : launch_status("fast_bwd_dsl_kernel (rect)");
}

// ---- the two-pass regime's rectangular blocks (exact-fp32 plans): U and Ut of this rank's rows against other ranks' columns ----------
// bf16 register-resident plans: two arrays of bf16 records (U, Ut) in the rectangular layout + (world + 1) x 2 bpad floats of zeros (the statistics
// of the side a launch must not weigh: W = U rz_p + Ut rz_q is formed as two rectangular launches of the saved backward)
static size_t rect_zero_floats(const crossclr_plan* plan) { return (size_t)(plan->world + 1) * 2 * plan->bpad; }
extern "C" size_t crossclr_rect_stash_bytes_s(const crossclr_plan* plan, int nranks) {
    if (!plan) return 0;
    const size_t one = crossclr_rect_stash_bytes(plan, nranks);
    if (plan->mode == CROSSCLR_MODE_BF16)
        return (one && rect_bytes_s(plan)) ? 2 * one + rect_zero_floats(plan) * 4 : 0;
    if (plan->fast_path || plan->mode != CROSSCLR_MODE_FP32) return 0;
    return one && 2 * one <= ((size_t)32 << 30) ? 2 * one : 0;
}

extern "C" int crossclr_forward_rect_save_s(const crossclr_plan* plan, const void* xhat_rows, const void* xhat_all, int first_rank,
                                            int nranks, float temperature, float negative_weight, const crossclr_sample_weights* sw,
                                            const float* shift_rows, const float* shift_all, float* part, int slot0, void* stash,
                                            void* stream) {
    if (!plan || !xhat_rows || !xhat_all || !shift_rows || !shift_all || !part || !stash) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (!crossclr_rect_stash_bytes_s(plan, nranks))
        return fail(CROSSCLR_E_ARG, "this plan has no two-pass save-for-backward path for remote blocks (crossclr_rect_stash_bytes_s == 0)");
    FwdSlot s;
    if (int rs = fwd_slot(plan, part, slot0, &s)) return rs;
    const float *krows, *kcols;
    if (int rk = unpack_k(sw, &krows, &kcols)) return rk;
    Geo g;
    int rc = rect_geo(plan, first_rank, nranks, temperature, negative_weight, &g, true);
    if (rc) return rc;
    if ((rc = device_zero_header(s.header, stream))) return rc;
    if (plan->mode == CROSSCLR_MODE_BF16) {
        rc = device_zero(static_cast<unsigned char*>(stash) + 2 * crossclr_rect_stash_bytes(plan, nranks), rect_zero_floats(plan) * 4, stream);
        if (rc) return rc;
    }
    return fwd_sums(plan, g, saving(full_pass(FwdPass::ShiftedSums, xhat_rows, xhat_all, s.out, kcols, shift_rows), stash, shift_all), stream);
}

extern "C" int crossclr_backward_rect_saved_s(const crossclr_plan* plan, const void* xhat_all, const void* stash, int first_rank,
                                              int nranks, float temperature, float negative_weight, const float* rz_rows,
                                              const float* wrz_rows, const float* rz_all, const float* wrz_all,
                                              const crossclr_sample_weights* sw, float* gbuf, int accumulate, void* stream) {
    if (!plan || !xhat_all || !stash || !rz_rows || !wrz_rows || !rz_all || !wrz_all || !gbuf) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (!crossclr_rect_stash_bytes_s(plan, nranks))
        return fail(CROSSCLR_E_ARG, "this plan has no two-pass save-for-backward path for remote blocks (crossclr_rect_stash_bytes_s == 0)");
    const float *krows, *kcols;
    Geo g;
    int rc = rect_saved_args(plan, sw, first_rank, nranks, temperature, negative_weight, true, &krows, &kcols, &g);
    if (rc) return rc;
    if (plan->mode == CROSSCLR_MODE_BF16) {
        // W[p][q] = U[p][q] rz_p + Ut[p][q] rz_q: two rectangular launches of the saved backward (saved_two_pass), no recompute
        const size_t one = crossclr_rect_stash_bytes(plan, nranks);
        const unsigned char* U = static_cast<const unsigned char*>(stash);
        const float* zeros = reinterpret_cast<const float*>(U + 2 * one);       // [world][2 bpad] for the column side, [2 bpad] of it for the rows
        return saved_two_pass(plan, xhat_all, {SavedBlock::Rect, g, U, "two-pass, rows' side"},
                              {SavedBlock::Rect, g, U + one, "two-pass, columns' side"}, zeros, rz_rows, wrz_rows, rz_all, wrz_all, krows, kcols,
                              gbuf, accumulate, "fast_bwd_dsl_kernel (rect, two-pass pair)", stream);
    }
    return launch_saved32<true, true>(plan, g, xhat_all, stash, rz_rows, wrz_rows, rz_all, wrz_all, krows, kcols, nranks * (2 * plan->bpad / 32),
                                      gbuf, accumulate, stream);
}


// The fragment-major copy of `nranks` consecutive packed operands (the slices of a gathered operand a rank received): what the pair
// kernel's rectangular launches read their column tiles from.
extern "C" int crossclr_pack_xf_from_packed(const crossclr_plan* plan, const void* xhat_packed, int nranks, void* xhat_xf, void* stream) {
    if (!plan || !xhat_packed || !xhat_xf || nranks < 1) return fail(CROSSCLR_E_ARG, "bad arguments");
    if (!plan->xf_bytes) return fail(CROSSCLR_E_ARG, "this plan has no fragment-major operand (xf_bytes == 0)");
    const size_t tiles = (size_t)nranks * 2 * plan->bpad / 32;
    if (tiles > 0x7fffffffull) return fail(CROSSCLR_E_ARG, "too many rows");
    LAUNCH(xf_from_packed_kernel, dim3((unsigned)tiles, (unsigned)((plan->Dpad + 1023) / 1024)), dim3(256), stream, (const bf16_t*)xhat_packed,
           (unsigned char*)xhat_xf, plan->Dpad);
    return launch_status("xf_from_packed_kernel");
}

// crossclr_backward_rect_saved on the fragment-major copy of the gathered operand, with the pair kernel (two tiles per barrier interval).
extern "C" int crossclr_backward_rect_saved_xfp(const crossclr_plan* plan, const void* xf_all, const void* stash, int first_rank,
                                                int nranks, float temperature, float negative_weight, const float* rz_rows,
                                                const float* wrz_rows, const float* rz_all, const float* wrz_all,
                                                const crossclr_sample_weights* sw, float* gbuf, int accumulate, void* stream) {
    if (!plan || !xf_all || !stash || !rz_rows || !wrz_rows || !rz_all || !wrz_all || !gbuf) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (!plan->stash_bytes || !plan->fast_path || !plan->xf_bytes) return fail(CROSSCLR_E_ARG, "this plan has no fragment-major saved backward for remote blocks");
    if ((size_t)plan->world * plan->operand_bytes >= ((size_t)1 << 32) || fast_stash_bytes_rect(plan->bpad, plan->Dpad, nranks) >= ((size_t)1 << 32))
        return fail(CROSSCLR_E_ARG, "crossclr_backward_rect_saved_xfp uses 32-bit offsets (operand / stash of 4 GiB or more): use crossclr_backward_rect_saved");
    const float *krows, *kcols;
    Geo g;
    int rc = rect_saved_args(plan, sw, first_rank, nranks, temperature, negative_weight, false, &krows, &kcols, &g);
    if (rc) return rc;
    rc = fast_backward_saved({SavedBlock::Rect, SavedOperand::FragmentPair}, plan, g, xf_all, stash, rz_rows, wrz_rows, rz_all, wrz_all, gbuf,
                             accumulate, krows, kcols, stream);
    return rc ? fail(rc, "fast_backward_saved (xfp, rect): unsupported Dpad %d", plan->Dpad) : launch_status("fast_bwd_xfp_kernel (rect)");
}

// The transpose of one saved rectangular block: what block (this rank x partner) contributes to the PARTNER's gradient buffer.
// crossclr_backward_rect_saved_t (RowMajor: this rank's packed operand) and _t_xfp (FragmentPair: its LOCAL fragment-major operand, what
// crossclr_normalize_xf wrote, with the pair kernel); fn: the entry point's name, for its refusals
static int backward_rect_saved_t(const char* fn, SavedOperand operand, const crossclr_plan* plan, const void* x_rows, const void* stash,
                                 int first_rank, int nranks, int which, float temperature, float negative_weight, const float* rz_rows,
                                 const float* wrz_rows, const float* rz_all, const float* wrz_all, const crossclr_sample_weights* sw,
                                 float* gpartner, void* stream) {
    if (!plan || !x_rows || !stash || !rz_rows || !wrz_rows || !rz_all || !wrz_all || !gpartner) return fail(CROSSCLR_E_ARG, "NULL argument");
    const bool pair = operand == SavedOperand::FragmentPair;
    if (!plan->stash_bytes || !plan->fast_path || (pair && !plan->xf_bytes))
        return fail(CROSSCLR_E_ARG, pair ? "this plan has no fragment-major saved backward for remote blocks"
                                         : "this plan has no save-for-backward path for remote blocks");
    if (which < 0 || which >= nranks) return fail(CROSSCLR_E_ARG, "which must be 0 .. nranks-1");
    if (pair && fast_stash_bytes_rect(plan->bpad, plan->Dpad, nranks) >= ((size_t)1 << 32))
        return fail(CROSSCLR_E_ARG, "%s uses 32-bit offsets (stash of 4 GiB or more): use crossclr_backward_rect_saved_t", fn);
    const float *krows, *kcols;
    Geo g;
    int rc = rect_saved_args(plan, sw, first_rank, nranks, temperature, negative_weight, false, &krows, &kcols, &g);     // (validates the range; scales)
    if (rc) return rc;
    // the kernel sees: rows = the partner's 2 bpad rows (statistics: its segment of the gathered arrays), columns = this rank's own rows
    const int partner = (first_rank + which) % plan->world;
    const size_t n2 = (size_t)2 * plan->bpad;
    rc = fast_backward_saved({SavedBlock::RectTransposed, operand}, plan, transposed_geo(plan, g, nranks, which, partner), x_rows, stash,
                             rz_all + partner * n2, wrz_all + partner * n2, rz_rows, wrz_rows, gpartner, 0,
                             kcols ? kcols + partner * n2 : nullptr, krows, stream);
    if (rc) return fail(rc, "fast_backward_saved%s: unsupported Dpad %d", pair ? " (xfp, transposed)" : "", plan->Dpad);
    return launch_status(pair ? "fast_bwd_xfp_kernel (rect, transposed)" : "fast_bwd_dsl_kernel (rect, transposed)");
}
extern "C" int crossclr_backward_rect_saved_t_xfp(const crossclr_plan* plan, const void* xf_rows, const void* stash, int first_rank,
                                                  int nranks, int which, float temperature, float negative_weight, const float* rz_rows,
                                                  const float* wrz_rows, const float* rz_all, const float* wrz_all,
                                                  const crossclr_sample_weights* sw, float* gpartner, void* stream) {
    return backward_rect_saved_t("crossclr_backward_rect_saved_t_xfp", SavedOperand::FragmentPair, plan, xf_rows, stash, first_rank, nranks, which,
                                 temperature, negative_weight, rz_rows, wrz_rows, rz_all, wrz_all, sw, gpartner, stream);
}
extern "C" int crossclr_backward_rect_saved_t(const crossclr_plan* plan, const void* xhat_rows, const void* stash, int first_rank,
                                              int nranks, int which, float temperature, float negative_weight, const float* rz_rows,
                                              const float* wrz_rows, const float* rz_all, const float* wrz_all,
                                              const crossclr_sample_weights* sw, float* gpartner, void* stream) {
    return backward_rect_saved_t("crossclr_backward_rect_saved_t", SavedOperand::RowMajor, plan, xhat_rows, stash, first_rank, nranks, which,
                                 temperature, negative_weight, rz_rows, wrz_rows, rz_all, wrz_all, sw, gpartner, stream);
}

// the recomputing backward over a (wrapping) rank range of the whole gathered operand: the blocks OTHER ranks evaluated in the
// pair scheme, whose exponentials this rank therefore does not hold
extern "C" int crossclr_backward_ranks(const crossclr_plan* plan, const void* xhat_rows, const void* xhat_all, int first_rank,
                                       int nranks, float temperature, float negative_weight, const float* rz_rows,
                                       const float* wrz_rows, const float* rz_all, const float* wrz_all,
                                       const crossclr_sample_weights* sw, float* gbuf, int accumulate, void* stream) {
    if (!plan || !xhat_rows || !xhat_all || !rz_rows || !wrz_rows || !rz_all || !wrz_all || !gbuf) return fail(CROSSCLR_E_ARG, "NULL argument");
    const float *krows, *kcols;
    if (int rk = unpack_k(sw, &krows, &kcols)) return rk;
    Geo g;
    int rc = rect_geo(plan, first_rank, nranks, temperature, negative_weight, &g);
    if (rc) return rc;
    if (plan->fast_bwd) {
        rc = plan->fast_bwd == 2
                 ? fast_backward16(plan, g, xhat_rows, xhat_all, rz_rows, wrz_rows, rz_all, wrz_all, gbuf, accumulate, krows, kcols, stream)
                 : fast_backward(plan, g, xhat_rows, xhat_all, rz_rows, wrz_rows, rz_all, wrz_all, gbuf, accumulate, krows, kcols, stream);
        return rc ? fail(rc, "fast backward: unsupported Dpad %d", plan->Dpad) : launch_status("fast_bwd_kernel (ranks)");
    }
    return with_plan_type<false>(plan, [&](auto t) {
        return backward_generic<typename decltype(t)::type>(plan, g, xhat_rows, xhat_all, rz_rows, wrz_rows, rz_all, wrz_all, gbuf, accumulate, krows,
                                                            kcols, nullptr, nullptr, stream);
    });
}

template <typename TIN>
static int backward_finish_t(const crossclr_plan* p, const float* gbuf, const void* v, const void* t, long ldv, long ldt,
                             const float* inv_norm, double inv_tau, const double* grad_out, void* gv, void* gt,
                             long ldgv, long ldgt, const float* lw, void* stream, int prenormalized = 0) {
    Geo g; memset(&g, 0, sizeof(g));
    g.b = p->b; g.bpad = p->bpad; g.D = p->D; g.Dpad = p->Dpad;
    dim3 grid((2 * p->b + 3) / 4), block(256);
    if (p->D <= 256 * kRowCache) {      // row pairs: each raw row read once
#define CROSSCLR_FINISH_PAIR(KC)                                                                                                        \
    LAUNCH((bwd_finish_pair_kernel<TIN, KC>), dim3((p->b + 3) / 4), block, stream, gbuf, p->bwd_slices, (const TIN*)v, (const TIN*)t, ldv, ldt, \
           g, inv_norm, inv_tau, p->b * p->world, grad_out, (TIN*)gv, (TIN*)gt, ldgv, ldgt, lw, prenormalized)
        switch ((p->D + 255) / 256) {      // (one instantiation per number of 256-element stretches a lane caches)
            case 1: CROSSCLR_FINISH_PAIR(1); break;
            case 2: CROSSCLR_FINISH_PAIR(2); break;
            case 3: CROSSCLR_FINISH_PAIR(3); break;
            default: CROSSCLR_FINISH_PAIR(4); break;
        }
#undef CROSSCLR_FINISH_PAIR
        return launch_status("bwd_finish_pair_kernel");
    }
    LAUNCH((bwd_finish_kernel<TIN>), grid, block, stream, gbuf, p->bwd_slices, (const TIN*)v, (const TIN*)t, ldv, ldt, g, inv_norm,
           inv_tau, p->b * p->world, grad_out, (TIN*)gv, (TIN*)gt, ldgv, ldgt, lw, prenormalized);
    return launch_status("bwd_finish_kernel");
}

extern "C" int crossclr_backward_finish(const crossclr_plan* plan, const float* gbuf, const void* video,
                                        const void* text, long ld_video, long ld_text, int in_dtype,
                                        const float* inv_norm, float temperature, const double* grad_out,
                                        void* grad_video, void* grad_text, long ld_gvideo, long ld_gtext,
                                        void* stream) {
    return crossclr_backward_finish_w(plan, gbuf, video, text, ld_video, ld_text, in_dtype, inv_norm, temperature, nullptr,
                                      grad_out, grad_video, grad_text, ld_gvideo, ld_gtext, stream);
}

extern "C" int crossclr_backward_finish_w(const crossclr_plan* plan, const float* gbuf, const void* video,
                                          const void* text, long ld_video, long ld_text, int in_dtype,
                                          const float* inv_norm, float temperature, const crossclr_sample_weights* sw,
                                          const double* grad_out, void* grad_video, void* grad_text, long ld_gvideo,
                                          long ld_gtext, void* stream) {
    return crossclr_backward_finish_p(plan, gbuf, video, text, ld_video, ld_text, in_dtype, inv_norm, temperature, sw, grad_out,
                                      grad_video, grad_text, ld_gvideo, ld_gtext, 0, stream);
}

// inv_tau: 1 / temperature as the kernels take it -- the float reciprocal of the float temperature for the loss (the value they have always
// been handed), 2 / B in full precision for the ranking loss, whose divisor B * B is no temperature and must not carry a float rounding
static int backward_finish_any(const crossclr_plan* plan, const float* gbuf, const void* video, const void* text, long ld_video, long ld_text,
                               int in_dtype, const float* inv_norm, double inv_tau, const float* lw, const double* grad_out, void* grad_video,
                               void* grad_text, long ld_gvideo, long ld_gtext, int prenormalized, void* stream) {
    if (!plan || !gbuf || !video || !text || !inv_norm || !grad_out || !grad_video || !grad_text)
        return fail(CROSSCLR_E_ARG, "NULL argument");
    return with_in_dtype(in_dtype, [&](auto tin) {
        return backward_finish_t<typename decltype(tin)::type>(plan, gbuf, video, text, ld_video, ld_text, inv_norm, inv_tau, grad_out, grad_video,
                                                               grad_text, ld_gvideo, ld_gtext, lw, stream, prenormalized);
    });
}

extern "C" int crossclr_backward_finish_p(const crossclr_plan* plan, const float* gbuf, const void* video,
                                          const void* text, long ld_video, long ld_text, int in_dtype,
                                          const float* inv_norm, float temperature, const crossclr_sample_weights* sw,
                                          const double* grad_out, void* grad_video, void* grad_text, long ld_gvideo,
                                          long ld_gtext, int prenormalized, void* stream) {
    if (!plan || !gbuf || !video || !text || !inv_norm || !grad_out || !grad_video || !grad_text)
        return fail(CROSSCLR_E_ARG, "NULL argument");
    if (!(temperature > 0.f)) return fail(CROSSCLR_E_ARG, "temperature must be > 0");
    return backward_finish_any(plan, gbuf, video, text, ld_video, ld_text, in_dtype, inv_norm, (double)(1.0f / temperature),
                               sw ? sw->loss_weight : nullptr, grad_out, grad_video, grad_text, ld_gvideo, ld_gtext, prenormalized, stream);
}

// ------------------------------------------------------------------------------------------------
// score statistics of the inter-modal block: max-margin ranking loss (trainer/loss.py:17-41) and retrieval ranks
static int score_geo(const crossclr_plan* p, float margin, Geo* g) {
    if (!p) return fail(CROSSCLR_E_ARG, "plan is NULL");
    if (p->world != 1) return fail(CROSSCLR_E_ARG, "score statistics are single-device (plan->world must be 1)");
    if (is_x3(p)) return refuse_x3("score statistics / max-margin");
    if (!isfinite(margin)) return fail(CROSSCLR_E_ARG, "margin must be finite");
    memset(g, 0, sizeof(*g));
    g->b = p->b; g->bpad = p->bpad; g->D = p->D; g->Dpad = p->Dpad;
    g->col_ranks = 1; g->col_rank0 = 0; g->row_rank = 0; g->skip_rank = -1; g->col_wrap = 0;
    g->c_inter = 1.f; g->c_intra = 1.f; g->m2 = margin;
    return CROSSCLR_OK;
}
extern "C" int crossclr_score_diag(const crossclr_plan* plan, const void* xhat, float* diag, void* stream) {
    if (!plan || !xhat || !diag) return fail(CROSSCLR_E_ARG, "NULL argument");
    Geo g;
    if (int rc = score_geo(plan, 0.f, &g)) return rc;
    const FwdSums d = full_pass(FwdPass::ScoreDiag, xhat, xhat, diag, nullptr, nullptr);
    return with_plan_type<false>(plan, [&](auto t) { return launch_fwd_sums<typename decltype(t)::type>(plan, g, d, stream); });
}

static int score_rows_impl(const crossclr_plan* plan, const void* xhat, const float* diag, float margin, float* part,
                           float* hinge, float* active, double* loss_sum, unsigned char* hinge_mask, void* stream) {
    if (!plan || !xhat || !diag || !part || !hinge || !active || !loss_sum) return fail(CROSSCLR_E_ARG, "NULL argument");
    Geo g;
    if (int rc = score_geo(plan, margin, &g)) return rc;
    if (plan->fwd_slots <= 0) return fail(CROSSCLR_E_ARG, "bad plan");
    float* cnt = part + (size_t)plan->fwd_slots * 2 * plan->bpad;     // launch group 1 of the forward workspace
    float* colpart = env_knobs().disable_symmetric ? nullptr : part + ws_colpart_off(plan);   // one pass for both directions
    // colpart: rows of modality 0 against the column tiles of modality 1, column statistics for the rest (the kernel's `header` argument is
    // free in this mode: it carries the optional hinge mask of crossclr_score_rows_save); else every row against every column tile
    FwdSums d = full_pass(FwdPass::ScoreRows, xhat, xhat, part, nullptr, diag);
    d.stash = cnt;
    if (colpart) { d.symmetric = true; d.header = reinterpret_cast<int*>(hinge_mask); d.colpart = colpart; }
    if (int rc = with_plan_type<false>(plan, [&](auto t) { return launch_fwd_sums<typename decltype(t)::type>(plan, g, d, stream); })) return rc;
    const int nb = plan->loss_ws_doubles - 1;
    LAUNCH(score_finish_kernel, dim3(nb), dim3(256), stream, (const float*)part, (const float*)cnt, plan->fwd_slots, plan->bpad, plan->b,
           hinge, active, loss_sum, (const float*)colpart);
    // loss_sum[0] = sum of the hinges, loss_sum[1] = the reference's mean: / (B * B)   (trainer/loss.py:41)
    LAUNCH(fwd_finish_reduce_kernel, dim3(1), dim3(64), stream, loss_sum, nb, 1.0 / ((double)plan->b * (double)plan->b));
    return launch_status("score_finish_kernel");
}
extern "C" int crossclr_score_rows(const crossclr_plan* plan, const void* xhat, const float* diag, float margin, float* part,
                                   float* hinge, float* active, double* loss_sum, void* stream) {
    return score_rows_impl(plan, xhat, diag, margin, part, hinge, active, loss_sum, nullptr, stream);
}
extern "C" size_t crossclr_maxmargin_mask_bytes(const crossclr_plan* plan) {
    if (!plan || plan->world != 1) return 0;
    return (size_t)plan->bpad * (size_t)plan->bpad;
}
extern "C" int crossclr_score_rows_save(const crossclr_plan* plan, const void* xhat, const float* diag, float margin, float* part,
                                        float* hinge, float* active, double* loss_sum, void* hinge_mask, void* stream) {
    if (!hinge_mask) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (env_knobs().disable_symmetric) return fail(CROSSCLR_E_ARG, "CROSSCLR_DISABLE_SYMMETRIC: the hinge mask is written by the one-pass evaluation only");
    return score_rows_impl(plan, xhat, diag, margin, part, hinge, active, loss_sum, static_cast<unsigned char*>(hinge_mask), stream);
}

template <typename T>
static int maxmargin_backward_t(const crossclr_plan* p, const Geo& g, const void* x, const float* diag, float* gbuf, void* stream) {
    const int tps = (2 * p->bpad / 64 + p->bwd_slices - 1) / p->bwd_slices;
    with_d_chunk<256, 128, 64>(p->Dpad, [&](auto dc) {
        constexpr int DC = decltype(dc)::value;
        LAUNCH((bwd_kernel<T, DC, false, false, 1>), bwd_grid(p, DC), dim3(256), stream, (const T*)x, (const T*)x, g, diag, diag, diag, diag, gbuf,
               0, tps, kNoF, kNoF, diag, diag);
    });
    return launch_status("bwd_kernel (max-margin)");
}

extern "C" int crossclr_maxmargin_backward(const crossclr_plan* plan, const void* xhat, const float* diag, float margin, float* gbuf,
                                           void* stream) {
    if (!plan || !xhat || !diag || !gbuf) return fail(CROSSCLR_E_ARG, "NULL argument");
    Geo g;
    if (int rc = score_geo(plan, margin, &g)) return rc;
    return with_plan_type<false>(plan, [&](auto t) { return maxmargin_backward_t<typename decltype(t)::type>(plan, g, xhat, diag, gbuf, stream); });
}

template <typename T>
static int maxmargin_backward_saved_t(const crossclr_plan* p, const Geo& g, const void* x, const unsigned char* mask, float* gbuf, void* stream) {
    const int tps = (2 * p->bpad / 64 + p->bwd_slices - 1) / p->bwd_slices;
    with_d_chunk<256, 128, 64>(p->Dpad, [&](auto dc) {
        constexpr int DC = decltype(dc)::value;
        LAUNCH((maxmargin_saved_kernel<T, DC>), bwd_grid(p, DC), dim3(256), stream, (const T*)x, g, mask, gbuf, tps);
    });
    return launch_status("maxmargin_saved_kernel");
}
extern "C" int crossclr_maxmargin_backward_saved(const crossclr_plan* plan, const void* xhat, const void* hinge_mask, float* gbuf, void* stream) {
    if (!plan || !xhat || !hinge_mask || !gbuf) return fail(CROSSCLR_E_ARG, "NULL argument");
    Geo g;
    if (int rc = score_geo(plan, 0.f, &g)) return rc;
    return with_plan_type<false>(plan, [&](auto t) {
        return maxmargin_backward_saved_t<typename decltype(t)::type>(plan, g, xhat, static_cast<const unsigned char*>(hinge_mask), gbuf, stream);
    });
}

extern "C" int crossclr_maxmargin_backward_finish(const crossclr_plan* plan, const float* gbuf, const void* im, const void* s,
                                                  long ld_im, long ld_s, int in_dtype, const float* ones, const float* active,
                                                  const double* grad_out, void* grad_im, void* grad_s, long ld_gim, long ld_gs,
                                                  void* stream) {
    if (!plan || !ones || !active) return fail(CROSSCLR_E_ARG, "NULL argument");
    // bwd_finish_kernel with unit rows as given: out = (sum_slices * inv_tau / (2B) - partner * inv_tau / B * (lw_im + lw_s) / 2) * grad_out;
    // inv_tau = 2 / B and lw = the active-hinge counts make that (sum_slices - (a_im + a_s) partner) / B^2   (loss.py:33-41)
    // (2 / B as a double: the float reciprocal of a float "temperature" B / 2 left the fp64 gradients with a relative error of 2^-24)
    return backward_finish_any(plan, gbuf, im, s, ld_im, ld_s, in_dtype, ones, 2.0 / (double)plan->b, active, grad_out, grad_im, grad_s, ld_gim,
                               ld_gs, 1, stream);
}

// ------------------------------------------------------------------------------------------------
// retrieval: fused similarity + top-k over two independent sets (crossclr_kernels_topk.h)
static int topk_mode_ok(int mode) { return mode == CROSSCLR_MODE_FP32 || mode == CROSSCLR_MODE_BF16 || mode == CROSSCLR_MODE_BF16X3; }
static int topk_set_ok(const char* what, int rows, int D) {
    if (rows < 1 || D < 1) return fail(CROSSCLR_E_ARG, "%s: empty set (rows=%d D=%d)", what, rows, D);
    if (rows > (1 << 30) || D > (1 << 20)) return fail(CROSSCLR_E_ARG, "%s: set too large (rows=%d D=%d)", what, rows, D);
    return CROSSCLR_OK;
}
static int topk_args_ok(const char* what, int nq, int ng, int D, int k) {
    if (int rc = topk_set_ok(what, nq, D)) return rc;
    if (int rc = topk_set_ok(what, ng, D)) return rc;
    if (k < 1) return fail(CROSSCLR_E_ARG, "%s: k must be at least 1 (got %d)", what, k);
    if (k > kTopkMaxK) return fail(CROSSCLR_E_ARG, "%s: k = %d is above the limit of %d (crossclr_topk_max_k)", what, k, kTopkMaxK);
    if (k > ng) return fail(CROSSCLR_E_ARG, "%s: k = %d is larger than the gallery (%d rows)", what, k, ng);
    return CROSSCLR_OK;
}
// column splits: enough thread blocks for two per CU of an MI355X (as the generic forward's grid), at most one per column tile, at most
// kTopkMaxCandidates / k (the merge kernel's list); `requested` > 0 replaces the first rule.  Every split owns at least one tile.
static int topk_splits(int nq, int ng, int k, int requested) {
    const int row_blocks = round_up(nq, kRowPad) / 128, ntiles = round_up(ng, kRowPad) / 128;
    int ns = requested > 0 ? requested : (512 + row_blocks - 1) / row_blocks;
    if (ns > kTopkMaxCandidates / k) ns = kTopkMaxCandidates / k;
    if (ns > ntiles) ns = ntiles;
    if (ns < 1) ns = 1;
    const int tps = (ntiles + ns - 1) / ns;
    return (ntiles + tps - 1) / tps;
}
extern "C" int crossclr_topk_max_k(void) { return kTopkMaxK; }
extern "C" size_t crossclr_topk_operand_bytes(int rows, int D, int mode) {
    if (rows < 1 || D < 1 || rows > (1 << 30) || D > (1 << 20) || !topk_mode_ok(mode)) return 0;
    return (size_t)round_up(rows, kRowPad) * (size_t)round_up(D, 64) * (mode == CROSSCLR_MODE_BF16 ? 2 : 4);
}
template <typename TIN>
static int topk_pack_t(const void* x, long ld, int rows, int D, int mode, int normalize, void* packed, void* stream) {
    const int rows_pad = round_up(rows, kRowPad), Dpad = round_up(D, 64);
    dim3 grid(rows_pad / 4), block(256);
#define CROSSCLR_LTP(TT) do { \
        if (normalize) LAUNCH((topk_pack_kernel<TIN, TT, true>), grid, block, stream, (const TIN*)x, ld, rows, rows_pad, D, Dpad, (TT*)packed); \
        else LAUNCH((topk_pack_kernel<TIN, TT, false>), grid, block, stream, (const TIN*)x, ld, rows, rows_pad, D, Dpad, (TT*)packed); } while (0)
    if (mode == CROSSCLR_MODE_FP32) CROSSCLR_LTP(float);
    else if (mode == CROSSCLR_MODE_BF16X3) CROSSCLR_LTP(x3_t);
    else CROSSCLR_LTP(bf16_t);
#undef CROSSCLR_LTP
    return launch_status("topk_pack_kernel");
}
extern "C" int crossclr_topk_pack(const void* x, long ld, int rows, int D, int in_dtype, int mode, int normalize, void* packed, void* stream) {
    if (!x || !packed) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (int rc = topk_set_ok("crossclr_topk_pack", rows, D)) return rc;
    if (!topk_mode_ok(mode)) return fail(CROSSCLR_E_ARG, "bad mode %d", mode);
    if (ld < D) return fail(CROSSCLR_E_ARG, "row stride smaller than D");
    return with_in_dtype(in_dtype,
                         [&](auto tin) { return topk_pack_t<typename decltype(tin)::type>(x, ld, rows, D, mode, normalize, packed, stream); });
}
extern "C" int crossclr_topk_splits(int nq, int ng, int k, int requested) {
    if (int rc = topk_args_ok("crossclr_topk_splits", nq, ng, 1, k)) return rc;
    return topk_splits(nq, ng, k, requested);
}
extern "C" size_t crossclr_topk_workspace_bytes(int nq, int ng, int k, int splits) {
    if (nq < 1 || ng < 1 || nq > (1 << 30) || ng > (1 << 30) || k < 1 || k > kTopkMaxK || k > ng) return 0;
    return (size_t)topk_splits(nq, ng, k, splits) * (size_t)round_up(nq, kRowPad) * (size_t)k * 8;
}
template <typename T>
static void topk_select_launch(const void* q, const void* g, int nq, int ng, int Dpad, int k, int ns, float* ws_s, int* ws_i, void* stream) {
    const int nq_pad = round_up(nq, kRowPad), ntiles = round_up(ng, kRowPad) / 128;
    const int tps = (ntiles + ns - 1) / ns;
    dim3 grid(nq_pad / 128, ns), block(256);
    if (k <= 16) LAUNCH((topk_select_kernel<T, 16>), grid, block, stream, (const T*)q, (const T*)g, nq, ng, nq_pad, Dpad, k, tps, ws_s, ws_i);
    else LAUNCH((topk_select_kernel<T, 64>), grid, block, stream, (const T*)q, (const T*)g, nq, ng, nq_pad, Dpad, k, tps, ws_s, ws_i);
}
extern "C" int crossclr_topk_select(const void* queries_packed, const void* gallery_packed, int nq, int ng, int D, int mode, int k, int splits,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!queries_packed || !gallery_packed || !workspace) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (int rc = topk_args_ok("crossclr_topk_select", nq, ng, D, k)) return rc;
    if (!topk_mode_ok(mode)) return fail(CROSSCLR_E_ARG, "bad mode %d", mode);
    const int ns = topk_splits(nq, ng, k, splits);
    const size_t entries = (size_t)ns * (size_t)round_up(nq, kRowPad) * (size_t)k;
    if (workspace_bytes < entries * 8)
        return fail(CROSSCLR_E_WORKSPACE, "crossclr_topk_select: workspace of %zu bytes, %zu needed (crossclr_topk_workspace_bytes)", workspace_bytes, entries * 8);
    float* ws_s = static_cast<float*>(workspace);
    int* ws_i = reinterpret_cast<int*>(ws_s + entries);
    const int Dpad = round_up(D, 64);
    if (mode == CROSSCLR_MODE_FP32) topk_select_launch<float>(queries_packed, gallery_packed, nq, ng, Dpad, k, ns, ws_s, ws_i, stream);
    else if (mode == CROSSCLR_MODE_BF16X3) topk_select_launch<x3_t>(queries_packed, gallery_packed, nq, ng, Dpad, k, ns, ws_s, ws_i, stream);
    else topk_select_launch<bf16_t>(queries_packed, gallery_packed, nq, ng, Dpad, k, ns, ws_s, ws_i, stream);
    return launch_status("topk_select_kernel");
}
extern "C" int crossclr_topk_merge(const void* workspace, int nq, int ng, int k, int splits, float* scores, int* indices, void* stream) {
    if (!workspace || !scores || !indices) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (int rc = topk_args_ok("crossclr_topk_merge", nq, ng, 1, k)) return rc;
    const int ns = topk_splits(nq, ng, k, splits), nq_pad = round_up(nq, kRowPad);
    const float* ws_s = static_cast<const float*>(workspace);
    const int* ws_i = reinterpret_cast<const int*>(ws_s + (size_t)ns * nq_pad * k);
    const int lpr = ns * k > 128 ? 256 : 64, rpb = 256 / lpr;      // long candidate lists: a whole block per row
    LAUNCH(topk_merge_kernel, dim3((nq + rpb - 1) / rpb), dim3(256), stream, ws_s, ws_i, nq, nq_pad, ns, k, lpr, scores, indices);
    return launch_status("topk_merge_kernel");
}

// ------------------------------------------------------------------------------------------------
// hardest negatives / maximum-violation ranking loss (crossclr_kernels_hardneg.h)
static int hardneg_plan_ok(const char* what, const crossclr_plan* p) {
    if (!p) return fail(CROSSCLR_E_ARG, "plan is NULL");
    if (p->world != 1) return fail(CROSSCLR_E_ARG, "%s: single-device (plan->world must be 1)", what);
    if (p->b < 1 || p->bpad < p->b || p->bpad % 128 != 0 || p->Dpad < 64 || p->Dpad % 64 != 0) return fail(CROSSCLR_E_ARG, "%s: bad plan", what);
    return CROSSCLR_OK;
}
// column splits: enough thread blocks for two per CU of an MI355X (the rule of crossclr_topk_splits), at most one per column tile;
// `requested` > 0 replaces the first rule.  Every split owns at least one tile.
static int hardneg_splits(const crossclr_plan* p, int requested) {
    const int ntiles = p->bpad / 128;
    int ns = requested > 0 ? requested : (512 + ntiles - 1) / ntiles;
    if (ns > ntiles) ns = ntiles;
    if (ns < 1) ns = 1;
    const int tps = (ntiles + ns - 1) / ns;
    return (ntiles + tps - 1) / tps;
}
// workspace, in 4-byte words: row scores [ns][bpad] | row indices [ns][bpad] | column scores [bpad / 128][bpad] | column rows, the same |
// positive-pair scores [bpad]
struct HardnegWs { float* row_s; int* row_i; float* col_s; int* col_i; float* pair; };
static size_t hardneg_ws_words(const crossclr_plan* p, int ns) { return ((size_t)2 * ns + (size_t)2 * (p->bpad / 128) + 1) * (size_t)p->bpad; }
static HardnegWs hardneg_ws(const crossclr_plan* p, int ns, void* workspace) {
    const size_t n = (size_t)p->bpad, nrb = (size_t)p->bpad / 128;
    float* w = static_cast<float*>(workspace);
    HardnegWs ws;
    ws.row_s = w;
    ws.row_i = reinterpret_cast<int*>(w + ns * n);
    ws.col_s = w + 2 * ns * n;
    ws.col_i = reinterpret_cast<int*>(w + (2 * ns + nrb) * n);
    ws.pair = w + (2 * ns + 2 * nrb) * n;
    return ws;
}
extern "C" int crossclr_hardneg_splits(const crossclr_plan* plan, int requested) {
    if (int rc = hardneg_plan_ok("crossclr_hardneg_splits", plan)) return rc;
    return hardneg_splits(plan, requested);
}
extern "C" size_t crossclr_hardneg_workspace_bytes(const crossclr_plan* plan, int splits) {
    if (hardneg_plan_ok("crossclr_hardneg_workspace_bytes", plan)) return 0;
    return hardneg_ws_words(plan, hardneg_splits(plan, splits)) * 4;
}
extern "C" int crossclr_hardneg_select(const crossclr_plan* plan, const void* xhat, int splits, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    if (int rc = hardneg_plan_ok("crossclr_hardneg_select", plan)) return rc;
    if (!xhat || !workspace) return fail(CROSSCLR_E_ARG, "NULL argument");
    const int ns = hardneg_splits(plan, splits);
    const size_t need = hardneg_ws_words(plan, ns) * 4;
    if (workspace_bytes < need)
        return fail(CROSSCLR_E_WORKSPACE, "crossclr_hardneg_select: workspace of %zu bytes, %zu needed (crossclr_hardneg_workspace_bytes)", workspace_bytes, need);
    const HardnegWs ws = hardneg_ws(plan, ns, workspace);
    const int ntiles = plan->bpad / 128, tps = (ntiles + ns - 1) / ns;
    return with_plan_type(plan, [&](auto t) {
        using T = typename decltype(t)::type;
        LAUNCH((hardneg_select_kernel<T>), dim3(ntiles, ns), dim3(256), stream, (const T*)xhat, plan->b, plan->bpad, plan->Dpad, tps, ws.row_s,
               ws.row_i, ws.col_s, ws.col_i, ws.pair);
        return launch_status("hardneg_select_kernel");
    });
}
extern "C" int crossclr_hardneg_finish(const crossclr_plan* plan, const void* workspace, int splits, float margin, int* best_index,
                                       float* best_score, float* hinge, float* pair_score, double* loss_sum, void* stream) {
    if (int rc = hardneg_plan_ok("crossclr_hardneg_finish", plan)) return rc;
    if (!workspace || !best_index || !best_score || !hinge || !pair_score || !loss_sum) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (!isfinite(margin)) return fail(CROSSCLR_E_ARG, "margin must be finite");
    const int ns = hardneg_splits(plan, splits);
    const HardnegWs ws = hardneg_ws(plan, ns, const_cast<void*>(workspace));
    const int nb = plan->loss_ws_doubles - 1;
    if (nb < 1) return fail(CROSSCLR_E_ARG, "bad plan");
    LAUNCH(hardneg_finish_kernel, dim3(nb), dim3(256), stream, (const float*)ws.row_s, (const int*)ws.row_i, ns, (const float*)ws.col_s,
           (const int*)ws.col_i, (const float*)ws.pair, plan->bpad, plan->b, margin, best_index, best_score, hinge, pair_score, loss_sum);
    // loss_sum[0] = sum of the 2 B hinges, loss_sum[1] = / (B * B): the sum form's divisor (trainer/loss.py:41)
    LAUNCH(fwd_finish_reduce_kernel, dim3(1), dim3(64), stream, loss_sum, nb, 1.0 / ((double)plan->b * (double)plan->b));
    return launch_status("hardneg_finish_kernel");
}
template <typename TIN>
static int hardneg_backward_t(const crossclr_plan* p, const void* im, const void* s, long ld_im, long ld_s, const int* best_index,
                              const float* hinge, const double* grad_out, void* grad_im, void* grad_s, long ld_gim, long ld_gs, void* stream) {
    LAUNCH((hardneg_backward_kernel<TIN>), dim3((p->b + 3) / 4, 2), dim3(256), stream, (const TIN*)im, (const TIN*)s, ld_im, ld_s, p->b, p->bpad,
           p->D, best_index, hinge, grad_out, (TIN*)grad_im, (TIN*)grad_s, ld_gim, ld_gs);
    return launch_status("hardneg_backward_kernel");
}
extern "C" int crossclr_hardneg_backward(const crossclr_plan* plan, const void* im, const void* s, long ld_im, long ld_s, int in_dtype,
                                         const int* best_index, const float* hinge, const double* grad_out, void* grad_im, void* grad_s,
                                         long ld_gim, long ld_gs, void* stream) {
    if (int rc = hardneg_plan_ok("crossclr_hardneg_backward", plan)) return rc;
    if (!im || !s || !best_index || !hinge || !grad_out || (!grad_im && !grad_s)) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (ld_im < plan->D || ld_s < plan->D || (grad_im && ld_gim < plan->D) || (grad_s && ld_gs < plan->D))
        return fail(CROSSCLR_E_ARG, "row stride smaller than D");
    return with_in_dtype(in_dtype, [&](auto tin) {
        return hardneg_backward_t<typename decltype(tin)::type>(plan, im, s, ld_im, ld_s, best_index, hinge, grad_out, grad_im, grad_s, ld_gim, ld_gs,
                                                                stream);
    });
}

// ------------------------------------------------------------------------------------------------
// pair_ids of the InfoNCE and the sigmoid loss (crossclr_kernels_pairids.h): int64 ids [b] -> int32 group [bpad] for the *_ids calls below
extern "C" int crossclr_pair_groups(const crossclr_plan* plan, const int64_t* ids, int32_t* group_out, void* stream) {
    if (int rc = hardneg_plan_ok("crossclr_pair_groups", plan)) return rc;
    if (!ids || !group_out) return fail(CROSSCLR_E_ARG, "crossclr_pair_groups: NULL argument");
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "id and group types");
    LAUNCH(pair_groups_kernel, dim3((plan->bpad + 255) / 256), dim3(256), stream, reinterpret_cast<const long long*>(ids), plan->b, plan->bpad,
           reinterpret_cast<int*>(group_out));
    return launch_status("pair_groups_kernel");
}

// ------------------------------------------------------------------------------------------------
// symmetric InfoNCE with a logit scale in device memory (crossclr_kernels_infonce.h).  Plans, column splits and the workspace's size are
// those of the hardest-negative pass: the same grid over the same tiles, (max, sum) pairs where that one keeps (score, index).
// workspace, in floats: row maxima [ns][bpad] | row sums [ns][bpad] | column maxima [bpad / 128][bpad] | column sums, the same |
// positive-pair scores [bpad]
struct InfonceWs { float* row_m; float* row_s; float* col_m; float* col_s; float* pair; };
static InfonceWs infonce_ws(const crossclr_plan* p, int ns, void* workspace) {
    const size_t n = (size_t)p->bpad, nrb = (size_t)p->bpad / 128;
    float* w = static_cast<float*>(workspace);
    return {w, w + ns * n, w + 2 * ns * n, w + (2 * ns + nrb) * n, w + (2 * ns + 2 * nrb) * n};
}
extern "C" int crossclr_infonce_splits(const crossclr_plan* plan, int requested) {
    if (int rc = hardneg_plan_ok("crossclr_infonce_splits", plan)) return rc;
    return hardneg_splits(plan, requested);
}
extern "C" size_t crossclr_infonce_workspace_bytes(const crossclr_plan* plan, int splits) {
    if (hardneg_plan_ok("crossclr_infonce_workspace_bytes", plan)) return 0;
    return hardneg_ws_words(plan, hardneg_splits(plan, splits)) * 4;
}
// `group` NULL: crossclr_infonce_stats; else crossclr_infonce_stats_ids (the same grid, workspace and split rule)
static int infonce_stats(const char* what, const crossclr_plan* plan, const void* xhat, const float* logit_scale, const int32_t* group, int splits,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = hardneg_plan_ok(what, plan)) return rc;
    if (!xhat || !logit_scale || !workspace) return fail(CROSSCLR_E_ARG, "NULL argument");
    const int ns = hardneg_splits(plan, splits);
    const size_t need = hardneg_ws_words(plan, ns) * 4;
    if (workspace_bytes < need)
        return fail(CROSSCLR_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (crossclr_infonce_workspace_bytes)", what, workspace_bytes, need);
    const InfonceWs ws = infonce_ws(plan, ns, workspace);
    const int ntiles = plan->bpad / 128, tps = (ntiles + ns - 1) / ns;
    return with_plan_type(plan, [&](auto t) {
        using T = typename decltype(t)::type;
        if (group) {
            LAUNCH((infonce_stats_kernel<T, true, const int*>), dim3(ntiles, ns), dim3(256), stream, (const T*)xhat, plan->b, plan->bpad, plan->Dpad, tps,
                   logit_scale, ws.row_m, ws.row_s, ws.col_m, ws.col_s, ws.pair, (const int*)group);
            return launch_status("infonce_stats_kernel<IDS>");
        }
        LAUNCH((infonce_stats_kernel<T>), dim3(ntiles, ns), dim3(256), stream, (const T*)xhat, plan->b, plan->bpad, plan->Dpad, tps, logit_scale,
               ws.row_m, ws.row_s, ws.col_m, ws.col_s, ws.pair);
        return launch_status("infonce_stats_kernel");
    });
}
extern "C" int crossclr_infonce_stats(const crossclr_plan* plan, const void* xhat, const float* logit_scale, int splits, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return infonce_stats("crossclr_infonce_stats", plan, xhat, logit_scale, nullptr, splits, workspace, workspace_bytes, stream);
}
extern "C" int crossclr_infonce_stats_ids(const crossclr_plan* plan, const void* xhat, const float* logit_scale, const int32_t* group, int splits,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!group) return fail(CROSSCLR_E_ARG, "crossclr_infonce_stats_ids: group is NULL (crossclr_pair_groups)");
    return infonce_stats("crossclr_infonce_stats_ids", plan, xhat, logit_scale, group, splits, workspace, workspace_bytes, stream);
}
extern "C" int crossclr_infonce_finish(const crossclr_plan* plan, const void* workspace, int splits, const float* logit_scale, float* lse,
                                       float* pair_score, double* loss_sum, void* stream) {
    if (int rc = hardneg_plan_ok("crossclr_infonce_finish", plan)) return rc;
    if (!workspace || !logit_scale || !lse || !pair_score || !loss_sum) return fail(CROSSCLR_E_ARG, "NULL argument");
    const int ns = hardneg_splits(plan, splits);
    const InfonceWs ws = infonce_ws(plan, ns, const_cast<void*>(workspace));
    const int nb = plan->loss_ws_doubles - 1;
    if (nb < 1) return fail(CROSSCLR_E_ARG, "bad plan");
    LAUNCH(infonce_finish_kernel, dim3(nb), dim3(256), stream, (const float*)ws.row_m, (const float*)ws.row_s, ns, (const float*)ws.col_m,
           (const float*)ws.col_s, (const float*)ws.pair, plan->bpad, plan->b, logit_scale, lse, pair_score, loss_sum);
    // loss_sum[0] = sum_i (lr[i] + lc[i] - 2 s S[i][i]), loss_sum[1] = that / (2 B)
    LAUNCH(fwd_finish_reduce_kernel, dim3(1), dim3(64), stream, loss_sum, nb, 0.5 / (double)plan->b);
    return launch_status("infonce_finish_kernel");
}
// The gradient product of the InfoNCE and the sigmoid loss (two kernels on one skeleton): the checks, the tiles per slice, the operand type
// and DC are the same for both; launch(type_tag<T>(), std::integral_constant<int, DC>(), tps) starts the loss's own kernel.
template <class F>
static int pairloss_backward(const char* what, const crossclr_plan* plan, bool args_ok, float* gbuf, const char* label, F launch) {
    if (int rc = hardneg_plan_ok(what, plan)) return rc;
    if (!args_ok || !gbuf) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (plan->bwd_slices < 1) return fail(CROSSCLR_E_ARG, "bad plan");
    const int tps = (plan->bpad / 64 + plan->bwd_slices - 1) / plan->bwd_slices;
    return with_plan_type(plan, [&](auto t) {
        with_d_chunk<256, 128, 64>(plan->Dpad, [&](auto dc) { launch(t, dc, tps); });
        return launch_status(label);
    });
}
// The gradient finish of both: g = s / (per_b B) M_p (per_b = 2 for InfoNCE, 1 for the sigmoid loss), dscale[0] = grad_out * sum_p <x^_p, M_p>
// over the 2 B stacked rows (= 2 sum_ij W S), dscale[1] = that times reduce_num / B = grad_out * dL/ds (1 / (4 B) and 1 / (2 B))
static int pairloss_backward_finish(const char* what, const crossclr_plan* plan, const float* gbuf, const void* video, const void* text,
                                    long ld_video, long ld_text, int in_dtype, const float* inv_norm, int normalized, const float* logit_scale,
                                    const double* grad_out, void* grad_video, void* grad_text, long ld_gvideo, long ld_gtext, double* dscale,
                                    double per_b, double reduce_num, void* stream) {
    if (int rc = hardneg_plan_ok(what, plan)) return rc;
    if (!gbuf || !video || !text || !logit_scale || !grad_out || !dscale || (normalized && !inv_norm)) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (plan->bwd_slices < 1 || plan->loss_ws_doubles < 2) return fail(CROSSCLR_E_ARG, "bad plan");
    if (ld_video < plan->D || ld_text < plan->D || (grad_video && ld_gvideo < plan->D) || (grad_text && ld_gtext < plan->D))
        return fail(CROSSCLR_E_ARG, "row stride smaller than D");
    const int nb = plan->loss_ws_doubles - 1;
    return with_in_dtype(in_dtype, [&](auto tin) {
        using TIN = typename decltype(tin)::type;
        LAUNCH((pairloss_backward_finish_kernel<TIN>), dim3(nb), dim3(256), stream, gbuf, plan->bwd_slices, (const TIN*)video, (const TIN*)text,
               ld_video, ld_text, plan->b, plan->bpad, plan->D, plan->Dpad, inv_norm, normalized, logit_scale, per_b * (double)plan->b, grad_out, (TIN*)grad_video,
               (TIN*)grad_text, ld_gvideo, ld_gtext, dscale);
        LAUNCH(fwd_finish_reduce_kernel, dim3(1), dim3(64), stream, dscale, nb, reduce_num / (double)plan->b);
        return launch_status("pairloss_backward_finish_kernel");
    });
}
static int infonce_backward(const char* what, const crossclr_plan* plan, const void* xhat, const float* logit_scale, const float* lse,
                            const float* pair_score, const int32_t* group, float* gbuf, void* stream) {
    return pairloss_backward(what, plan, xhat && logit_scale && lse && pair_score, gbuf,
                             group ? "infonce_backward_kernel<IDS>" : "infonce_backward_kernel", [&](auto t, auto dc, int tps) {
        using T = typename decltype(t)::type;
        constexpr int DC = decltype(dc)::value;
        if (group)
            LAUNCH((infonce_backward_kernel<T, DC, true, const int*>), bwd_grid(plan, DC), dim3(256), stream, (const T*)xhat, plan->b, plan->bpad, plan->Dpad,
                   logit_scale, lse, pair_score, gbuf, tps, (const int*)group);
        else
            LAUNCH((infonce_backward_kernel<T, DC>), bwd_grid(plan, DC), dim3(256), stream, (const T*)xhat, plan->b, plan->bpad, plan->Dpad,
                   logit_scale, lse, pair_score, gbuf, tps);
    });
}
extern "C" int crossclr_infonce_backward(const crossclr_plan* plan, const void* xhat, const float* logit_scale, const float* lse,
                                         const float* pair_score, float* gbuf, void* stream) {
    return infonce_backward("crossclr_infonce_backward", plan, xhat, logit_scale, lse, pair_score, nullptr, gbuf, stream);
}
extern "C" int crossclr_infonce_backward_ids(const crossclr_plan* plan, const void* xhat, const float* logit_scale, const float* lse,
                                             const float* pair_score, const int32_t* group, float* gbuf, void* stream) {
    if (!group) return fail(CROSSCLR_E_ARG, "crossclr_infonce_backward_ids: group is NULL (crossclr_pair_groups)");
    return infonce_backward("crossclr_infonce_backward_ids", plan, xhat, logit_scale, lse, pair_score, group, gbuf, stream);
}
extern "C" int crossclr_infonce_backward_finish(const crossclr_plan* plan, const float* gbuf, const void* video, const void* text, long ld_video,
                                                long ld_text, int in_dtype, const float* inv_norm, int normalized, const float* logit_scale,
                                                const double* grad_out, void* grad_video, void* grad_text, long ld_gvideo, long ld_gtext,
                                                double* dscale, void* stream) {
    return pairloss_backward_finish("crossclr_infonce_backward_finish", plan, gbuf, video, text, ld_video, ld_text, in_dtype, inv_norm, normalized,
                                    logit_scale, grad_out, grad_video, grad_text, ld_gvideo, ld_gtext, dscale, 2.0, 0.25, stream);
}

// ------------------------------------------------------------------------------------------------
// pairwise sigmoid loss with a logit scale and a logit bias in device memory (crossclr_kernels_sigmoid.h).  Plans and column splits are
// those of the hardest-negative pass; there is no column side.
// workspace, in floats: row softplus sums [ns][bpad] | row sigmoid sums [ns][bpad] | positive-pair scores [bpad]
struct SigmoidWs { float* row_sp; float* row_sig; float* pair; };
static size_t sigmoid_ws_words(const crossclr_plan* p, int ns) { return ((size_t)2 * ns + 1) * (size_t)p->bpad; }
static SigmoidWs sigmoid_ws(const crossclr_plan* p, int ns, void* workspace) {
    const size_t n = (size_t)p->bpad;
    float* w = static_cast<float*>(workspace);
    return {w, w + ns * n, w + 2 * ns * n};
}
extern "C" int crossclr_sigmoid_splits(const crossclr_plan* plan, int requested) {
    if (int rc = hardneg_plan_ok("crossclr_sigmoid_splits", plan)) return rc;
    return hardneg_splits(plan, requested);
}
extern "C" size_t crossclr_sigmoid_workspace_bytes(const crossclr_plan* plan, int splits) {
    if (hardneg_plan_ok("crossclr_sigmoid_workspace_bytes", plan)) return 0;
    return sigmoid_ws_words(plan, hardneg_splits(plan, splits)) * 4;
}
// `group` NULL: crossclr_sigmoid_stats; else crossclr_sigmoid_stats_ids (the same grid, workspace and split rule)
static int sigmoid_stats(const char* what, const crossclr_plan* plan, const void* xhat, const float* logit_scale, const float* logit_bias,
                         const int32_t* group, int splits, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = hardneg_plan_ok(what, plan)) return rc;
    if (!xhat || !logit_scale || !logit_bias || !workspace) return fail(CROSSCLR_E_ARG, "NULL argument");
    const int ns = hardneg_splits(plan, splits);
    const size_t need = sigmoid_ws_words(plan, ns) * 4;
    if (workspace_bytes < need)
        return fail(CROSSCLR_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (crossclr_sigmoid_workspace_bytes)", what, workspace_bytes, need);
    const SigmoidWs ws = sigmoid_ws(plan, ns, workspace);
    const int ntiles = plan->bpad / 128, tps = (ntiles + ns - 1) / ns;
    return with_plan_type(plan, [&](auto t) {
        using T = typename decltype(t)::type;
        if (group) {
            LAUNCH((sigmoid_stats_kernel<T, true, const int*>), dim3(ntiles, ns), dim3(256), stream, (const T*)xhat, plan->b, plan->bpad, plan->Dpad, tps,
                   logit_scale, logit_bias, ws.row_sp, ws.row_sig, ws.pair, (const int*)group);
            return launch_status("sigmoid_stats_kernel<IDS>");
        }
        LAUNCH((sigmoid_stats_kernel<T>), dim3(ntiles, ns), dim3(256), stream, (const T*)xhat, plan->b, plan->bpad, plan->Dpad, tps, logit_scale,
               logit_bias, ws.row_sp, ws.row_sig, ws.pair);
        return launch_status("sigmoid_stats_kernel");
    });
}
extern "C" int crossclr_sigmoid_stats(const crossclr_plan* plan, const void* xhat, const float* logit_scale, const float* logit_bias, int splits,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    return sigmoid_stats("crossclr_sigmoid_stats", plan, xhat, logit_scale, logit_bias, nullptr, splits, workspace, workspace_bytes, stream);
}
extern "C" int crossclr_sigmoid_stats_ids(const crossclr_plan* plan, const void* xhat, const float* logit_scale, const float* logit_bias,
                                          const int32_t* group, int splits, void* workspace, size_t workspace_bytes, void* stream) {
    if (!group) return fail(CROSSCLR_E_ARG, "crossclr_sigmoid_stats_ids: group is NULL (crossclr_pair_groups)");
    return sigmoid_stats("crossclr_sigmoid_stats_ids", plan, xhat, logit_scale, logit_bias, group, splits, workspace, workspace_bytes, stream);
}
extern "C" int crossclr_sigmoid_finish(const crossclr_plan* plan, const void* workspace, int splits, const float* logit_scale,
                                       const float* logit_bias, float* row_loss, float* pair_score, double* loss_sum, double* sig_sum,
                                       void* stream) {
    if (int rc = hardneg_plan_ok("crossclr_sigmoid_finish", plan)) return rc;
    if (!workspace || !logit_scale || !logit_bias || !row_loss || !pair_score || !loss_sum || !sig_sum) return fail(CROSSCLR_E_ARG, "NULL argument");
    const int ns = hardneg_splits(plan, splits);
    const SigmoidWs ws = sigmoid_ws(plan, ns, const_cast<void*>(workspace));
    const int nb = plan->loss_ws_doubles - 1;
    if (nb < 1) return fail(CROSSCLR_E_ARG, "bad plan");
    LAUNCH(sigmoid_finish_kernel, dim3(nb), dim3(256), stream, (const float*)ws.row_sp, (const float*)ws.row_sig, ns, (const float*)ws.pair,
           plan->bpad, plan->b, logit_scale, logit_bias, row_loss, pair_score, loss_sum, sig_sum);
    // loss_sum[0] = sum_i row_loss[i], loss_sum[1] = that / B;  sig_sum[0] = sum_ij W[i][j], sig_sum[1] = that / B = dL/dbeta
    LAUNCH(fwd_finish_reduce_kernel, dim3(1), dim3(64), stream, loss_sum, nb, 1.0 / (double)plan->b);
    LAUNCH(fwd_finish_reduce_kernel, dim3(1), dim3(64), stream, sig_sum, nb, 1.0 / (double)plan->b);
    return launch_status("sigmoid_finish_kernel");
}
static int sigmoid_backward(const char* what, const crossclr_plan* plan, const void* xhat, const float* logit_scale, const float* logit_bias,
                            const int32_t* group, float* gbuf, void* stream) {
    return pairloss_backward(what, plan, xhat && logit_scale && logit_bias, gbuf,
                             group ? "sigmoid_backward_kernel<IDS>" : "sigmoid_backward_kernel", [&](auto t, auto dc, int tps) {
        using T = typename decltype(t)::type;
        constexpr int DC = decltype(dc)::value;
        if (group)
            LAUNCH((sigmoid_backward_kernel<T, DC, true, const int*>), bwd_grid(plan, DC), dim3(256), stream, (const T*)xhat, plan->b, plan->bpad, plan->Dpad,
                   logit_scale, logit_bias, gbuf, tps, (const int*)group);
        else
            LAUNCH((sigmoid_backward_kernel<T, DC>), bwd_grid(plan, DC), dim3(256), stream, (const T*)xhat, plan->b, plan->bpad, plan->Dpad,
                   logit_scale, logit_bias, gbuf, tps);
    });
}
extern "C" int crossclr_sigmoid_backward(const crossclr_plan* plan, const void* xhat, const float* logit_scale, const float* logit_bias,
                                         float* gbuf, void* stream) {
    return sigmoid_backward("crossclr_sigmoid_backward", plan, xhat, logit_scale, logit_bias, nullptr, gbuf, stream);
}
extern "C" int crossclr_sigmoid_backward_ids(const crossclr_plan* plan, const void* xhat, const float* logit_scale, const float* logit_bias,
                                             const int32_t* group, float* gbuf, void* stream) {
    if (!group) return fail(CROSSCLR_E_ARG, "crossclr_sigmoid_backward_ids: group is NULL (crossclr_pair_groups)");
    return sigmoid_backward("crossclr_sigmoid_backward_ids", plan, xhat, logit_scale, logit_bias, group, gbuf, stream);
}
extern "C" int crossclr_sigmoid_backward_finish(const crossclr_plan* plan, const float* gbuf, const void* video, const void* text, long ld_video,
                                                long ld_text, int in_dtype, const float* inv_norm, int normalized, const float* logit_scale,
                                                const double* grad_out, void* grad_video, void* grad_text, long ld_gvideo, long ld_gtext,
                                                double* dscale, void* stream) {
    return pairloss_backward_finish("crossclr_sigmoid_backward_finish", plan, gbuf, video, text, ld_video, ld_text, in_dtype, inv_norm, normalized,
                                    logit_scale, grad_out, grad_video, grad_text, ld_gvideo, ld_gtext, dscale, 1.0, 0.5, stream);
}

// ------------------------------------------------------------------------------------------------
// influential-sample statistics
template <typename TIN>
static int infl_colsum_t(const void* xv, const void* xt, long ldv, long ldt, int b, int Din, float* inv_norm, float* partial,
                         double* colsum, void* stream) {
#define CROSSCLR_LI(KC) LAUNCH((infl_colsum_kernel<TIN, KC>), dim3(kInflBlocks, 2), dim3(256), stream, (const TIN*)xv, (const TIN*)xt, ldv, ldt, b, Din, inv_norm, partial)
    if (Din <= 256) CROSSCLR_LI(1);
    else if (Din <= 512) CROSSCLR_LI(2);
    else if (Din <= 1024) CROSSCLR_LI(4);
    else if (Din <= 2048) CROSSCLR_LI(8);
    else CROSSCLR_LI(16);
#undef CROSSCLR_LI
    LAUNCH(infl_colsum_finish_kernel, dim3((Din + 63) / 64, 2), dim3(256), stream, (const float*)partial, kInflBlocks, Din, colsum);
    return launch_status("infl_colsum_kernel");
}
template <typename TIN>
static int infl_conn_t(const void* xv, const void* xt, long ldv, long ldt, int b, int Din, const float* inv_norm,
                       const double* colsum, int Bglobal, double* conn, void* stream) {
    LAUNCH((infl_conn_kernel<TIN>), dim3((b + 3) / 4, 2), dim3(256), stream, (const TIN*)xv, (const TIN*)xt, ldv, ldt, b, Din,
           inv_norm, colsum, Bglobal, conn);
    return launch_status("infl_conn_kernel");
}
static int infl_args(const void* xv, const void* xt, long ldv, long ldt, int b, int Din) {
    if (!xv || !xt) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (b < 1 || Din < 1 || Din > CROSSCLR_INFL_MAX_DIN) return fail(CROSSCLR_E_ARG, "need b >= 1 and 1 <= Din <= %d", CROSSCLR_INFL_MAX_DIN);
    if (ldv < Din || ldt < Din) return fail(CROSSCLR_E_ARG, "row stride smaller than Din");
    return CROSSCLR_OK;
}

extern "C" int crossclr_influence_colsum(const void* x_video, const void* x_text, long ld_video, long ld_text, int in_dtype,
                                         int b, int Din, float* inv_norm, float* partial_ws, double* colsum, void* stream) {
    static_assert(kInflBlocks == CROSSCLR_INFL_BLOCKS && 256 * kInflMaxCols == CROSSCLR_INFL_MAX_DIN, "header out of sync");
    if (int rc = infl_args(x_video, x_text, ld_video, ld_text, b, Din)) return rc;
    if (!inv_norm || !partial_ws || !colsum) return fail(CROSSCLR_E_ARG, "NULL argument");
    return with_in_dtype(in_dtype, [&](auto tin) {
        return infl_colsum_t<typename decltype(tin)::type>(x_video, x_text, ld_video, ld_text, b, Din, inv_norm, partial_ws, colsum, stream);
    });
}

extern "C" int crossclr_influence_conn(const void* x_video, const void* x_text, long ld_video, long ld_text, int in_dtype,
                                       int b, int Din, const float* inv_norm, const double* colsum_total, int B_global,
                                       double* conn, void* stream) {
    if (int rc = infl_args(x_video, x_text, ld_video, ld_text, b, Din)) return rc;
    if (!inv_norm || !colsum_total || !conn || B_global < b) return fail(CROSSCLR_E_ARG, "NULL argument / B_global < b");
    return with_in_dtype(in_dtype, [&](auto tin) {
        return infl_conn_t<typename decltype(tin)::type>(x_video, x_text, ld_video, ld_text, b, Din, inv_norm, colsum_total, B_global, conn, stream);
    });
}

extern "C" int crossclr_influence_finish(const crossclr_plan* plan, const double* conn_all, float score_threshold,
                                         float temperature_weights, float* neg_scale, float* loss_weight, void* stream) {
    if (!plan || !conn_all || !neg_scale || !loss_weight) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (!(temperature_weights > 0.f)) return fail(CROSSCLR_E_ARG, "temperature_weights must be > 0");
    LAUNCH(infl_finish_kernel, dim3(2), dim3(1024), stream, conn_all, plan->world, plan->rank, plan->b, plan->bpad,
           (double)score_threshold, (double)temperature_weights, neg_scale, loss_weight);
    return launch_status("infl_finish_kernel");
}

// The sustained rate of the bf16 matrix pipe on THIS device, measured in the run that quotes it (bench.py: `roofline.sustained_mfma`):
// 256 blocks x 4 waves (one per SIMD), 16 independent accumulator chains of v_mfma_f32_32x32x16_bf16 per wave, nothing else in the
// loop; operands pseudo-random (toggling data: what the package power limit allows a real kernel) or all zero (`zero_operands`).
// One launch executes blocks * 4 * iters * 16 MFMAs of 32768 flop.
namespace crossclr {
#ifndef CROSSCLR_EMU
__global__ void __launch_bounds__(256, 1) mfma_sustained_kernel(float* out, int iters, unsigned seed, int zero_operands) {
    f32x16 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    unsigned x = seed + threadIdx.x * 2654435761u + blockIdx.x * 40503u;
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        x = x * 1664525u + 1013904223u;
        a[j] = zero_operands ? (__bf16)0.f : (__bf16)((float)(x >> 8) * (1.f / 16777216.f) - 0.5f);
        x = x * 1664525u + 1013904223u;
        b[j] = zero_operands ? (__bf16)0.f : (__bf16)((float)(x >> 8) * (1.f / 16777216.f) - 0.5f);
    }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = mfma_32x32x16_bf16(a, b, acc[i]);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc[i][r];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}
#endif
}  // namespace crossclr

// ------------------------------------------------------------------------------------------------
// The whole step behind two calls (include/crossclr.h, ABI 6 / 7): the kernel-selection policy that used to live in the Python module.
// Composition of the entry points above.  crossclr_step_plan decides everything -- it is the only one of the three that reads the
// environment -- and writes the decision into the layout; forward and backward act on the layout they are handed (sealed with a check word).
static size_t step_max_stash_bytes() {
    const char* e = getenv("CROSSCLR_MAX_STASH_GB");
    double gb = 8.0;
    if (e) {
        char* end = nullptr;
        const double v = strtod(e, &end);
        if (end != e && isfinite(v)) gb = v < 0.0 ? 0.0 : (v > 1024.0 ? 1024.0 : v);      // (garbage: the default; negative: no stash)
    }
    return (size_t)(gb * (double)((size_t)1 << 30));
}
// Padded widths at which the fragment-major saved backward beats the LDS-staged one (profiles/r03_xf_widths.txt: wins from 512 up, ties at
// 384, loses at 256 / 128), with the row floor below which crossclr_normalize_xf's second copy is not paid back; CROSSCLR_XF_WIDTHS="128,256"
// (or "") overrides the widths and drops the floor (tuning / tests)
static bool step_use_xf(const crossclr_plan* p) {
    const char* e = getenv("CROSSCLR_XF_WIDTHS");
    if (!e) {
        static const int widths[] = {512, 768, 1024, 1152, 1536, 2048, 2560, 3072, 4096, 5120, 6144, 8192};
        bool in = false;
        for (int w : widths) in = in || p->Dpad == w;
        return in && p->bpad >= (p->Dpad <= 512 ? 2048 : 4096);
    }
    for (const char* c = e; *c;) {
        char* end;
        const long w = strtol(c, &end, 10);
        if (end == c) { ++c; continue; }
        if (w == p->Dpad) return true;
        c = end;
    }
    return false;
}
static size_t step_align(size_t x) { return (x + 255) / 256 * 256; }
// FNV-1a over the plan and every layout field in front of `check`: a layout the library did not write for this plan is refused
static unsigned step_check(const crossclr_plan* plan, const crossclr_step_layout* L) {
    unsigned h = 2166136261u;
    auto mix = [&](const void* p, size_t n) {
        const unsigned char* c = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 16777619u;
    };
    // (field by field: struct padding is not part of the value)
    const int pi[] = {plan->b, plan->D, plan->world, plan->rank, plan->mode, plan->bpad, plan->Dpad, plan->fast_path, plan->fast_bwd,
                      plan->fwd_blocks, plan->fwd_slots, plan->bwd_slices, plan->loss_ws_doubles};
    const size_t pz[] = {plan->fwd_ws_floats, plan->operand_bytes, plan->gbuf_bytes, plan->stash_bytes, plan->xf_bytes};
    const size_t lz[] = {L->total_bytes, L->persistent_bytes, L->transient_bytes, L->backward_scratch_bytes, L->xhat, L->inv_norm, L->diag,
                         L->logz, L->rz, L->wrz, L->part, L->shift, L->xf, L->stash, L->gbuf, L->ticket, L->stash_bytes, L->xf_bytes};
    const int li[] = {(int)L->flags, L->two_pass, L->saved, L->backward_kernel};
    mix(pi, sizeof(pi)); mix(pz, sizeof(pz)); mix(lz, sizeof(lz)); mix(li, sizeof(li));
    mix(&L->temperature, sizeof(float)); mix(&L->negative_weight, sizeof(float));
    return h ? h : 1u;
}

extern "C" int crossclr_step_plan(const crossclr_plan* plan, float temperature, float negative_weight, unsigned flags,
                                  size_t workspace_bytes, crossclr_step_layout* L) {
    if (!plan || !L) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (plan->world != 1) return fail(CROSSCLR_E_ARG, "crossclr_step_* is the single-device step (plan->world == 1); sharded runs compose the fine-grained entry points around their collectives");
    if (!(temperature > 0.f) || !isfinite(temperature) || !isfinite(negative_weight)) return fail(CROSSCLR_E_ARG, "temperature must be > 0 and finite, negative_weight finite");
    const bool two_pass = needs_row_shift(temperature, negative_weight);
    const bool fwd_only = (flags & CROSSCLR_STEP_FORWARD_ONLY) != 0;
    const bool may_save = !(flags & (CROSSCLR_STEP_NO_SAVE | CROSSCLR_STEP_FORWARD_ONLY));
    const bool eager = (flags & CROSSCLR_STEP_EAGER) && !fwd_only;
    const size_t stash_full = two_pass ? crossclr_stash_bytes_s(plan) : plan->stash_bytes;
    const size_t max_stash = step_max_stash_bytes();
    for (int attempt = 0; attempt < 2; ++attempt) {
        const bool saved = attempt == 0 && may_save && stash_full > 0 && stash_full <= max_stash;
        if (attempt == 0 && !saved) continue;
        // which saved backward: the fragment-major copy is only laid out (and written by the forward's first kernel) when a kernel that reads it is allowed
        int backward_kernel = saved ? 1 : 0;
        if (saved && !two_pass && plan->xf_bytes > 0 && step_use_xf(plan)) {
            const char* e = getenv("CROSSCLR_XFP");
            const bool xfp_ok = plan->stash_bytes < ((size_t)1 << 32) && !(e && e[0] == '0') && !(flags & CROSSCLR_STEP_NO_XFP);
            const bool xf1_ok = plan->Dpad <= 1024 && !(flags & CROSSCLR_STEP_NO_XF);     // (wide plans: the pair kernel or the LDS-staged one)
            backward_kernel = xfp_ok ? 3 : (xf1_ok ? 2 : 1);
        }
        const bool xf = backward_kernel >= 2;
        memset(L, 0, sizeof(*L));
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t o = off; off += step_align(bytes); return o; };
        const size_t n2 = (size_t)2 * plan->bpad;
        L->shift = L->xf = L->stash = L->gbuf = CROSSCLR_STEP_NONE;
        // region 1 (persistent): what the backward call reads
        if (eager) {                    // the finish kernel alone: 1 / ||x|| and the gradient slices
            L->inv_norm = take(4 * n2);
            L->gbuf = take(plan->gbuf_bytes);
        } else if (!fwd_only) {         // the gradient product (from saved exponentials, or recomputed: also what a backward without `transient` does)
            L->xhat = take(plan->operand_bytes);
            L->inv_norm = take(4 * n2);
            L->rz = take(4 * n2);
            L->wrz = take(4 * n2);
            if (two_pass) L->shift = take(4 * n2);
        }
        L->persistent_bytes = off;
        // region 2 (transient)
        if (eager || fwd_only) {
            L->xhat = take(plan->operand_bytes);
            if (fwd_only) L->inv_norm = take(4 * n2);
            L->rz = take(4 * n2);
            L->wrz = take(4 * n2);
            if (two_pass) L->shift = take(4 * n2);
        }
        L->diag = take(4 * (size_t)plan->bpad);
        L->logz = take(4 * n2);
        L->part = take(4 * plan->fwd_ws_floats);
        L->ticket = take(4);
        if (xf) L->xf = take(plan->xf_bytes);
        if (saved) L->stash = take(stash_full);
        L->xf_bytes = xf ? plan->xf_bytes : 0;
        L->stash_bytes = saved ? stash_full : 0;
        L->total_bytes = off;
        L->transient_bytes = off - L->persistent_bytes;
        L->backward_scratch_bytes = (fwd_only || eager) ? 0 : plan->gbuf_bytes;
        L->temperature = temperature;
        L->negative_weight = negative_weight;
        L->flags = flags;
        L->two_pass = two_pass ? 1 : 0;
        L->saved = saved ? 1 : 0;
        L->backward_kernel = backward_kernel;
        L->check = step_check(plan, L);
        if (workspace_bytes == 0 || off <= workspace_bytes) return CROSSCLR_OK;
    }
    return fail(CROSSCLR_E_WORKSPACE, "workspace of %zu bytes is below the recomputing layout's %zu", workspace_bytes, L->total_bytes);
}

namespace {
struct StepBufs {
    crossclr_step_layout L;
    unsigned char *persistent, *transient;
    unsigned char* at(size_t off) const {
        if (off == CROSSCLR_STEP_NONE) return nullptr;
        if (off < L.persistent_bytes) return persistent + off;
        return transient ? transient + (off - L.persistent_bytes) : nullptr;
    }
    void* xhat() const { return at(L.xhat); }
    float* f(size_t off) const { return reinterpret_cast<float*>(at(off)); }
    void* v(size_t off) const { return at(off); }
};
}  // namespace
static int step_bind(const crossclr_plan* plan, const crossclr_step_layout* layout, void* persistent, void* transient, bool transient_needed,
                     StepBufs* B) {
    if (!plan || !layout) return fail(CROSSCLR_E_ARG, "NULL argument");
    if (layout->check == 0 || layout->check != step_check(plan, layout))
        return fail(CROSSCLR_E_ARG, "this crossclr_step_layout was not written by crossclr_step_plan for this plan (or was modified since)");
    if (layout->persistent_bytes > 0 && !persistent) return fail(CROSSCLR_E_ARG, "persistent is NULL (layout.persistent_bytes = %zu)", layout->persistent_bytes);
    if (transient_needed && layout->transient_bytes > 0 && !transient) return fail(CROSSCLR_E_ARG, "transient is NULL (layout.transient_bytes = %zu)", layout->transient_bytes);
    B->L = *layout;
    B->persistent = static_cast<unsigned char*>(persistent);
    B->transient = static_cast<unsigned char*>(transient);
    return CROSSCLR_OK;
}
static int step_gradient_product(const crossclr_plan* plan, const StepBufs& B, const float* k, float* gbuf, bool from_saved, void* stream);

extern "C" int crossclr_step_forward(const crossclr_plan* plan, const crossclr_step_layout* layout, const void* video, const void* text,
                                     long ld_video, long ld_text, int in_dtype, const crossclr_sample_weights* sw,
                                     void* persistent, void* transient, double* loss_ws, void* stream) {
    if (!loss_ws || !video || !text) return fail(CROSSCLR_E_ARG, "NULL argument");
    StepBufs B;
    if (int rc = step_bind(plan, layout, persistent, transient, true, &B)) return rc;
    const crossclr_step_layout& L = B.L;
    const float temperature = L.temperature, negative_weight = L.negative_weight;
    const unsigned flags = L.flags;
    const float* k = sw ? sw->neg_scale_rows : nullptr;
    const float* lw = sw ? sw->loss_weight : nullptr;
    const crossclr_sample_weights sw_k = {k, k, nullptr}, sw_klw = {k, k, lw};
    const crossclr_sample_weights* pk = k ? &sw_k : nullptr;
    const crossclr_sample_weights* pklw = (k || lw) ? &sw_klw : nullptr;
    const bool pre = (flags & CROSSCLR_STEP_PRENORMALIZED) != 0;
    int rc;
    // loss.py:79-80 (+ the packed operand, 1 / ||x||, the positive pairs' cosines; with a fragment-major saved backward to follow: its operand copy)
    int* ticket = reinterpret_cast<int*>(B.at(L.ticket));      // cleared by this first kernel, taken by the finish kernel's blocks
    if (L.xf != CROSSCLR_STEP_NONE)
        rc = pre ? normalize_xf_any<false>(plan, video, text, ld_video, ld_text, in_dtype, B.xhat(), B.v(L.xf), B.f(L.inv_norm), B.f(L.diag), stream, ticket)
                 : normalize_xf_any<true>(plan, video, text, ld_video, ld_text, in_dtype, B.xhat(), B.v(L.xf), B.f(L.inv_norm), B.f(L.diag), stream, ticket);
    else
        rc = pre ? normalize_any<false>(plan, video, text, ld_video, ld_text, in_dtype, B.xhat(), B.f(L.inv_norm), B.f(L.diag), stream, ticket)
                 : normalize_any<true>(plan, video, text, ld_video, ld_text, in_dtype, B.xhat(), B.f(L.inv_norm), B.f(L.diag), stream, ticket);
    if (rc) return rc;
    if (L.two_pass) {      // loss.py:60's float64 soft-max takes the row maximum; so do these: row maxima, then sums relative to them
        rc = crossclr_forward_rowmax(plan, B.xhat(), B.xhat(), 1, plan->rank, -1, temperature, negative_weight, pk, B.f(L.part), B.f(L.shift), 0, stream);
        if (rc) return rc;
        rc = L.saved ? crossclr_forward_save_s(plan, B.xhat(), temperature, negative_weight, pk, B.f(L.shift), B.f(L.part), 0, B.v(L.stash), stream)
                     : crossclr_forward_s(plan, B.xhat(), B.xhat(), 1, plan->rank, -1, temperature, negative_weight, pk, B.f(L.shift), B.f(L.part), 0, stream);
        if (rc) return rc;
        rc = forward_finish_impl(plan, B.f(L.part), plan->fwd_slots, B.f(L.diag), temperature, negative_weight, pklw, B.f(L.shift),
                                 B.f(L.logz), B.f(L.rz), B.f(L.wrz), loss_ws, stream, ticket);
        if (rc || L.gbuf == CROSSCLR_STEP_NONE) return rc;
        return step_gradient_product(plan, B, k, B.f(L.gbuf), L.saved != 0, stream);
    }
    // loss.py:83-100, 59-60: soft-max denominators of the local block (and, saving, its exponentials)
    rc = L.saved ? crossclr_forward_save(plan, B.xhat(), temperature, negative_weight, pk, B.f(L.part), 0, B.v(L.stash), stream)
                 : crossclr_forward_w(plan, B.xhat(), B.xhat(), 1, plan->rank, -1, temperature, negative_weight, pk, B.f(L.part), 0, stream);
    if (rc) return rc;
    // loss.py:60 (-log), :111-114
    rc = forward_finish_impl(plan, B.f(L.part), plan->fwd_slots, B.f(L.diag), temperature, negative_weight, pklw, nullptr, B.f(L.logz), B.f(L.rz),
                             B.f(L.wrz), loss_ws, stream, ticket);
    if (rc || L.gbuf == CROSSCLR_STEP_NONE) return rc;
    return step_gradient_product(plan, B, k, B.f(L.gbuf), L.saved != 0, stream);      // CROSSCLR_STEP_EAGER
}

// autograd of loss.py:83-112: gbuf = d(loss)/d(unit rows), unscaled, in column slices (independent of grad_out).
// from_saved = false: the recomputing product (a step that did not save, or a backward whose caller has released the transient region)
static int step_gradient_product(const crossclr_plan* plan, const StepBufs& B, const float* k, float* gbuf, bool from_saved, void* stream) {
    const crossclr_step_layout& L = B.L;
    const float temperature = L.temperature, negative_weight = L.negative_weight;
    const crossclr_sample_weights sw_k = {k, k, nullptr};
    const crossclr_sample_weights* pk = k ? &sw_k : nullptr;
    float *rz = B.f(L.rz), *wrz = B.f(L.wrz);
    if (L.two_pass)
        return from_saved ? crossclr_backward_saved_s(plan, B.xhat(), B.v(L.stash), temperature, negative_weight, rz, wrz, pk, gbuf, 0, stream)
                          : crossclr_backward_s(plan, B.xhat(), B.xhat(), 1, plan->rank, -1, temperature, negative_weight, rz, wrz, rz, wrz, pk,
                                                B.f(L.shift), B.f(L.shift), gbuf, 0, stream);
    if (from_saved) {
        switch (L.backward_kernel) {
            case 3: return crossclr_backward_saved_xfp(plan, B.v(L.xf), B.v(L.stash), temperature, negative_weight, rz, wrz, pk, gbuf, 0, stream);
            case 2: return crossclr_backward_saved_xf(plan, B.v(L.xf), B.v(L.stash), temperature, negative_weight, rz, wrz, pk, gbuf, 0, stream);
            default: return crossclr_backward_saved(plan, B.xhat(), B.v(L.stash), temperature, negative_weight, rz, wrz, pk, gbuf, 0, stream);
        }
    }
    return crossclr_backward_w(plan, B.xhat(), B.xhat(), 1, plan->rank, -1, temperature, negative_weight, rz, wrz, rz, wrz, pk, gbuf, 0, stream);
}

extern "C" int crossclr_step_backward(const crossclr_plan* plan, const crossclr_step_layout* layout, const void* video, const void* text,
                                      long ld_video, long ld_text, int in_dtype, const crossclr_sample_weights* sw,
                                      void* persistent, void* transient, void* scratch, const double* grad_out,
                                      void* grad_video, void* grad_text, long ld_gvideo, long ld_gtext, void* stream) {
    if (!video || !text || !grad_out || !grad_video || !grad_text) return fail(CROSSCLR_E_ARG, "NULL argument");
    StepBufs B;
    if (int rc = step_bind(plan, layout, persistent, transient, false, &B)) return rc;
    const crossclr_step_layout& L = B.L;
    if (L.flags & CROSSCLR_STEP_FORWARD_ONLY) return fail(CROSSCLR_E_ARG, "the forward of this step was declared CROSSCLR_STEP_FORWARD_ONLY");
    const float* k = sw ? sw->neg_scale_rows : nullptr;
    const float* lw = sw ? sw->loss_weight : nullptr;
    const crossclr_sample_weights sw_lw = {nullptr, nullptr, lw};
    float* gbuf;
    if (L.gbuf != CROSSCLR_STEP_NONE) {
        gbuf = B.f(L.gbuf);                 // CROSSCLR_STEP_EAGER: the forward call enqueued the gradient product already
    } else {
        if (!scratch) return fail(CROSSCLR_E_ARG, "scratch is NULL (layout.backward_scratch_bytes bytes)");
        gbuf = static_cast<float*>(scratch);
        // (transient == NULL: released after an earlier backward through this step -- everything the recomputing product reads is persistent)
        if (int rc = step_gradient_product(plan, B, k, gbuf, L.saved != 0 && transient != nullptr, stream)) return rc;
    }
    // autograd of loss.py:79-80 + the positive-pair term, x grad_out, in the input dtype
    return crossclr_backward_finish_p(plan, gbuf, video, text, ld_video, ld_text, in_dtype, B.f(L.inv_norm), L.temperature, lw ? &sw_lw : nullptr, grad_out,
                                      grad_video, grad_text, ld_gvideo, ld_gtext, (L.flags & CROSSCLR_STEP_PRENORMALIZED) ? 1 : 0, stream);
}

// ------------------------------------------------------------------------------------------------
// Second-order terms (include/crossclr.h, ABI 7; crossclr_kernels_hvp.h): what autograd's double backward through loss.py:79-114 computes,
// composed of the exact-fp32 first-order entry points above and the two passes of hvp_kernel.
namespace {
struct HvpLayout {
    size_t xhat, vhat, inv_norm, diag, logz, rz, wrz, shift, drz, dwrz, part, loss_ws, gbuf1, dzpart, gbuf2, dgo_rows, total;
    int nz;
};
}  // namespace
static int hvp_layout(const crossclr_plan* plan, HvpLayout* H) {
    if (!plan) return fail(CROSSCLR_E_ARG, "plan is NULL");
    if (plan->world != 1) return fail(CROSSCLR_E_ARG, "crossclr_second_order is single-device (plan->world == 1)");
    if (plan->mode != CROSSCLR_MODE_FP32 || plan->fast_path) return fail(CROSSCLR_E_ARG, "crossclr_second_order takes a CROSSCLR_MODE_FP32 plan (second-order terms are formed from exact-fp32 products)");
    const size_t n2 = (size_t)2 * plan->bpad;
    const int rb = 2 * plan->bpad / 64, ntiles = 2 * plan->bpad / 64;
    int nz = (1024 + rb - 1) / rb;
    if (nz > ntiles) nz = ntiles;
    if (nz > 16) nz = 16;
    if (nz < 1) nz = 1;
    H->nz = nz;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += step_align(bytes); return o; };
    H->xhat = take(plan->operand_bytes);
    H->vhat = take(plan->operand_bytes);
    H->inv_norm = take(4 * n2);
    H->diag = take(4 * (size_t)plan->bpad);
    H->logz = take(4 * n2);
    H->rz = take(4 * n2);
    H->wrz = take(4 * n2);
    H->shift = take(4 * n2);
    H->drz = take(4 * n2);
    H->dwrz = take(4 * n2);
    H->part = take(4 * plan->fwd_ws_floats);
    H->loss_ws = take(8 * (size_t)(plan->loss_ws_doubles > 2 ? plan->loss_ws_doubles : 2));
    H->gbuf1 = take(plan->gbuf_bytes);
    H->dzpart = take(4 * (size_t)nz * n2);
    H->gbuf2 = take(4 * (size_t)nz * n2 * plan->Dpad);
    H->dgo_rows = take(8 * n2);
    H->total = off;
    return CROSSCLR_OK;
}
extern "C" size_t crossclr_second_order_workspace_bytes(const crossclr_plan* plan) {
    HvpLayout H;
    return hvp_layout(plan, &H) ? 0 : H.total;
}

template <typename TIN>
static int second_order_impl(const crossclr_plan* plan, const HvpLayout& H, const Geo& g, const TIN* video, const TIN* text, long ldv, long ldt,
                             float temperature, float negative_weight, const float* k, const float* lw, int prenormalized, bool two_pass,
                             const TIN* uvideo, const TIN* utext, long lduv, long ldut, const double* grad_out, unsigned char* w,
                             TIN* hvideo, TIN* htext, long ldhv, long ldht, double* d_grad_out, void* stream) {
    auto F = [&](size_t off) { return reinterpret_cast<float*>(w + off); };
    const int n2 = 2 * plan->bpad;
    const float* shift = two_pass ? F(H.shift) : nullptr;
    // v = the tangent of the unit rows along u
    LAUNCH((hvp_tangent_kernel<TIN>), dim3((unsigned)((n2 + 3) / 4)), dim3(256), stream, video, text, ldv, ldt, uvideo, utext, lduv, ldut, g,
           F(H.inv_norm), prenormalized, F(H.vhat));
    if (int rc = launch_status("hvp_tangent_kernel")) return rc;
    const int rb = n2 / 64, ntiles = n2 / 64;
    const int tps = (ntiles + H.nz - 1) / H.nz;
    const float* X = F(H.xhat);
    const float* V = F(H.vhat);
    // pass 1: dZ, then the tangents of omega / Z
    if (k) LAUNCH((hvp_kernel<64, true, 1>), dim3(rb, 1, H.nz), dim3(256), stream, X, V, g, F(H.rz), F(H.wrz), kNoF, kNoF, k, shift, F(H.dzpart), tps);
    else LAUNCH((hvp_kernel<64, false, 1>), dim3(rb, 1, H.nz), dim3(256), stream, X, V, g, F(H.rz), F(H.wrz), kNoF, kNoF, kNoF, shift, F(H.dzpart), tps);
    if (int rc = launch_status("hvp_kernel (row sums)")) return rc;
    LAUNCH(hvp_stats_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), stream, F(H.dzpart), H.nz, n2, F(H.rz), lw, negative_weight, F(H.drz), F(H.dwrz));
    if (int rc = launch_status("hvp_stats_kernel")) return rc;
    // pass 2: dG in column slices
#define CROSSCLR_LH(DC, NS)                                                                                                                          \
    do {                                                                                                                                             \
        if (k) LAUNCH((hvp_kernel<DC, true, 2, NS>), dim3(rb, plan->Dpad / (DC * NS), H.nz), dim3(256), stream, X, V, g, F(H.rz), F(H.wrz), F(H.drz), \
                      F(H.dwrz), k, shift, F(H.gbuf2), tps);                                                                                         \
        else LAUNCH((hvp_kernel<DC, false, 2, NS>), dim3(rb, plan->Dpad / (DC * NS), H.nz), dim3(256), stream, X, V, g, F(H.rz), F(H.wrz), F(H.drz),  \
                    F(H.dwrz), kNoF, shift, F(H.gbuf2), tps);                                                                                        \
    } while (0)
    // (two 256-column slices per block where they divide the row: S and T of a tile are evaluated once for 512 output columns)
    if (plan->Dpad % 512 == 0) CROSSCLR_LH(256, 2);
    else if (plan->Dpad % 256 == 0) CROSSCLR_LH(256, 1);
    else if (plan->Dpad % 128 == 0) CROSSCLR_LH(128, 1);
    else CROSSCLR_LH(64, 1);
#undef CROSSCLR_LH
    if (int rc = launch_status("hvp_kernel (product)")) return rc;
    // the row-local chain: normalisation, positive pairs, x grad_out; and <u, dL/d(rows)>
    double* dgo_rows = reinterpret_cast<double*>(w + H.dgo_rows);
    LAUNCH((hvp_finish_kernel<TIN>), dim3((unsigned)((2 * plan->b + 3) / 4)), dim3(256), stream, F(H.gbuf1), plan->bwd_slices, F(H.gbuf2), H.nz, video, text,
           ldv, ldt, uvideo, utext, lduv, ldut, g, F(H.inv_norm), 1.f / temperature, plan->b * plan->world, grad_out, lw, prenormalized, hvideo, htext,
           ldhv, ldht, dgo_rows);
    if (int rc = launch_status("hvp_finish_kernel")) return rc;
    LAUNCH(hvp_reduce_kernel, dim3(1), dim3(64), stream, dgo_rows, 2 * plan->b, d_grad_out);
    return launch_status("hvp_reduce_kernel");
}

extern "C" int crossclr_second_order(const crossclr_plan* plan, const void* video, const void* text, long ld_video, long ld_text, int in_dtype,
                                     float temperature, float negative_weight, const crossclr_sample_weights* sw, int prenormalized,
                                     const void* u_video, const void* u_text, long ld_uvideo, long ld_utext, const double* grad_out,
                                     void* workspace, size_t workspace_bytes, void* h_video, void* h_text, long ld_hvideo, long ld_htext,
                                     double* d_grad_out, void* stream) {
    if (!video || !text || !u_video || !u_text || !grad_out || !workspace || !h_video || !h_text || !d_grad_out) return fail(CROSSCLR_E_ARG, "NULL argument");
    HvpLayout H;
    if (int rc = hvp_layout(plan, &H)) return rc;
    if (workspace_bytes < H.total) return fail(CROSSCLR_E_WORKSPACE, "workspace of %zu bytes, crossclr_second_order_workspace_bytes says %zu", workspace_bytes, H.total);
    if (prenormalized != 0 && prenormalized != 1) return fail(CROSSCLR_E_ARG, "prenormalized must be 0 or 1");
    if (ld_video < plan->D || ld_text < plan->D || ld_uvideo < plan->D || ld_utext < plan->D || ld_hvideo < plan->D || ld_htext < plan->D)
        return fail(CROSSCLR_E_ARG, "row stride smaller than D");
    unsigned char* w = static_cast<unsigned char*>(workspace);
    auto F = [&](size_t off) { return reinterpret_cast<float*>(w + off); };
    const float* k = sw ? sw->neg_scale_rows : nullptr;
    const float* lw = sw ? sw->loss_weight : nullptr;
    const crossclr_sample_weights sw_k = {k, k, nullptr}, sw_klw = {k, k, lw};
    const crossclr_sample_weights* pk = k ? &sw_k : nullptr;
    const crossclr_sample_weights* pklw = (k || lw) ? &sw_klw : nullptr;
    const bool two_pass = needs_row_shift(temperature, negative_weight);
    Geo g;
    if (int rc = make_geo(plan, 1, plan->rank, -1, temperature, negative_weight, &g, true)) return rc;
    // the first-order pieces, exact fp32: unit rows, soft-max statistics, the gradient product (loss.py:79-112 and its autograd)
    int rc = prenormalized ? normalize_any<false>(plan, video, text, ld_video, ld_text, in_dtype, w + H.xhat, F(H.inv_norm), F(H.diag), stream)
                           : normalize_any<true>(plan, video, text, ld_video, ld_text, in_dtype, w + H.xhat, F(H.inv_norm), F(H.diag), stream);
    if (rc) return rc;
    double* loss_ws = reinterpret_cast<double*>(w + H.loss_ws);
    if (two_pass) {
        rc = crossclr_forward_rowmax(plan, w + H.xhat, w + H.xhat, 1, plan->rank, -1, temperature, negative_weight, pk, F(H.part), F(H.shift), 0, stream);
        if (rc) return rc;
        rc = crossclr_forward_s(plan, w + H.xhat, w + H.xhat, 1, plan->rank, -1, temperature, negative_weight, pk, F(H.shift), F(H.part), 0, stream);
        if (rc) return rc;
        rc = forward_finish_impl(plan, F(H.part), plan->fwd_slots, F(H.diag), temperature, negative_weight, pklw, F(H.shift), F(H.logz), F(H.rz), F(H.wrz),
                                 loss_ws, stream, nullptr);
        if (rc) return rc;
        rc = crossclr_backward_s(plan, w + H.xhat, w + H.xhat, 1, plan->rank, -1, temperature, negative_weight, F(H.rz), F(H.wrz), F(H.rz), F(H.wrz), pk,
                                 F(H.shift), F(H.shift), F(H.gbuf1), 0, stream);
    } else {
        rc = crossclr_forward_w(plan, w + H.xhat, w + H.xhat, 1, plan->rank, -1, temperature, negative_weight, pk, F(H.part), 0, stream);
        if (rc) return rc;
        rc = forward_finish_impl(plan, F(H.part), plan->fwd_slots, F(H.diag), temperature, negative_weight, pklw, nullptr, F(H.logz), F(H.rz), F(H.wrz),
                                 loss_ws, stream, nullptr);
        if (rc) return rc;
        rc = crossclr_backward_w(plan, w + H.xhat, w + H.xhat, 1, plan->rank, -1, temperature, negative_weight, F(H.rz), F(H.wrz), F(H.rz), F(H.wrz), pk,
                                 F(H.gbuf1), 0, stream);
    }
    if (rc) return rc;
    return with_in_dtype(in_dtype, [&](auto tin) {
        using TIN = typename decltype(tin)::type;
        return second_order_impl<TIN>(plan, H, g, (const TIN*)video, (const TIN*)text, ld_video, ld_text, temperature, negative_weight, k, lw,
                                      prenormalized, two_pass, (const TIN*)u_video, (const TIN*)u_text, ld_uvideo, ld_utext, grad_out, w,
                                      (TIN*)h_video, (TIN*)h_text, ld_hvideo, ld_htext, d_grad_out, stream);
    });
}

extern "C" int crossclr_mfma_sustained(float* out, int blocks, int iters, unsigned seed, int zero_operands, void* stream) {
#ifndef CROSSCLR_EMU
    if (!out || blocks < 1 || blocks > 4096 || iters < 1) return fail(CROSSCLR_E_ARG, "bad mfma_sustained arguments");
    LAUNCH(mfma_sustained_kernel, dim3(blocks), dim3(256), stream, out, iters, seed, zero_operands);
    return launch_status("mfma_sustained_kernel");
#else
    (void)out; (void)blocks; (void)iters; (void)seed; (void)zero_operands; (void)stream;
    return fail(CROSSCLR_E_ARG, "crossclr_mfma_sustained measures the device: not available in the host emulation");
#endif
}

extern "C" int crossclr_selftest(int which, const void* in, void* out, void* stream) {
    if (which < 0 || which > 4 || !in || !out) return fail(CROSSCLR_E_ARG, "bad selftest arguments");
    LAUNCH(selftest_kernel, dim3(1), dim3(64), stream, which, in, out);
    return launch_status("selftest_kernel");
}

#ifdef CROSSCLR_TIMING
// (variant builds only; not declared in include/crossclr.h) the marks of the most recent pipelined launch: [blocks][8] uint64
extern "C" int crossclr_debug_timing(unsigned long long* host_out, int nblocks) {
    if (!host_out || nblocks < 1 || nblocks > 1024) return fail(CROSSCLR_E_ARG, "bad timing request");
    if (hipDeviceSynchronize() != hipSuccess) return fail(CROSSCLR_E_HIP, "synchronize failed");
    if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_timing), sizeof(unsigned long long) * 8 * (size_t)nblocks) != hipSuccess)
        return fail(CROSSCLR_E_HIP, "reading the timing marks failed");
    return CROSSCLR_OK;
}
#endif
