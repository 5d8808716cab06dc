// plan.hip -- host-side engine of libst3d: error reporting, the frozen VGG-19 weight store
// (utils.py:48-52) and the fused perceptual-loss plan (losses.py:12-44 /
// style_transfer.py:59-83): forward to conv5_1 keeping the post-ReLU taps, Gram + content
// losses, and the hand-scheduled backward to d loss / d image.  The graph is static, so the
// backward is a fixed launch sequence over preallocated workspaces (no autograd tape, no
// allocation per step); what the reference recomputes every call but does not depend on the
// optimised parameters (content features, style Grams: losses.py:18-25) is set once through
// st3d_plan_set_content / st3d_plan_set_style.
#include <stdarg.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "epochs.h"
#include "planlists.h"

namespace st3d {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace st3d

extern "C" int st3d_version(void) { return 100; }
extern "C" const char *st3d_last_error(void) { return st3d::g_err; }

extern "C" int st3d_device_info(int device, int *cu_count, size_t *hbm_bytes, char *name, int name_len) {
    hipDeviceProp_t p;
    ST3D_HIP(hipGetDeviceProperties(&p, device));
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = p.totalGlobalMem;
    if (name && name_len > 0) {
        snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
    }
    return ST3D_OK;
}

using namespace st3d;      // the VGG layout, the route table and the list decisions (planlists.h)

namespace {

// style taps (style_transfer.py:12-19 minus conv4_2) and the content tap
const int kStyleTap[5] = {0, 5, 10, 19, 28};
constexpr int kContentTap = 21;

}  // namespace

struct st3d_vgg {
    float *wf[16];     // direct implicit-GEMM packs (conv.hip)
    float *wd[16];
    float *uf[16];     // Winograd packs (wino.hip), nullptr where the layer shape is not supported
    float *ud[16];
    float *u6f[16];    // Winograd F(4x4,3x3) packs (wino43.hip), nullptr where not supported
    float *u6d[16];
    int wino43_mink;   // layers with at least this many input channels (K of the GEMM) run F(4x4,3x3) where the shape allows;
                       // 0 = never (ST3D_WINO43=0); ST3D_WINO43_MINK overrides the measured default
    float *bias[16];
    bool set[16];
    bool use_wino;     // ST3D_CONV=direct forces the direct kernels (A/B runs)
    bool pregate;      // ST3D_PREGATE=0: every input-gradient launch applies its own ReLU gate (A/B runs)
    bool fuse_tap0;    // ST3D_TAP0_FUSED=0: relu1_1 Gram backward and conv1_1 input gradient as separate launches (A/B runs)
    uint64_t sets;     // st3d_vgg_set_conv calls so far: a plan that remembers what its buffers hold remembers this with it
};

extern "C" int st3d_vgg_create(st3d_vgg **out) {
    ST3D_CHECK_ARG(out);
    st3d_vgg *v = new st3d_vgg();
    memset(v, 0, sizeof(*v));
    const char *mode = getenv("ST3D_CONV");
    v->use_wino = !(mode && strcmp(mode, "direct") == 0);
    const char *t0 = getenv("ST3D_TAP0_FUSED");
    v->fuse_tap0 = !(t0 && t0[0] == '0');
    const char *pg = getenv("ST3D_PREGATE");
    v->pregate = !(pg && pg[0] == '0');
    const char *w6 = getenv("ST3D_WINO43"), *w6k = getenv("ST3D_WINO43_MINK");
    v->wino43_mink = (w6 && w6[0] == '0') ? 0 : (w6k ? atoi(w6k) : 64);
    for (int i = 0; i < 16; ++i) {
        const size_t n = st3d_conv3x3_packed_floats(kConvCout[i], kConvCin[i]);
        bool ok = hipMalloc(&v->wf[i], n * sizeof(float)) == hipSuccess && hipMalloc(&v->wd[i], n * sizeof(float)) == hipSuccess &&
                  hipMalloc(&v->bias[i], kConvCout[i] * sizeof(float)) == hipSuccess;
        // both directions must be Winograd-able (dgrad swaps the channel roles)
        if (ok && st3d_wino_supported(kConvCin[i], kConvCout[i], 4, 4) && st3d_wino_supported(kConvCout[i], kConvCin[i], 4, 4)) {
            const size_t nu = st3d_wino_packed_floats(kConvCout[i], kConvCin[i]);
            ok = hipMalloc(&v->uf[i], nu * sizeof(float)) == hipSuccess && hipMalloc(&v->ud[i], nu * sizeof(float)) == hipSuccess;
        }
        if (ok && v->use_wino && v->wino43_mink > 0 && kConvCin[i] % 64 == 0 && kConvCout[i] % 64 == 0 &&
            (kConvCin[i] >= v->wino43_mink || kConvCout[i] >= v->wino43_mink)) {
            const size_t nu = st3d_wino43_packed_floats(kConvCout[i], kConvCin[i]);
            ok = hipMalloc(&v->u6f[i], nu * sizeof(float)) == hipSuccess && hipMalloc(&v->u6d[i], nu * sizeof(float)) == hipSuccess;
        }
        if (!ok) {
            st3d::set_error("st3d_vgg_create: hipMalloc failed");
            st3d_vgg_destroy(v);
            return ST3D_E_NOMEM;
        }
    }
    *out = v;
    return ST3D_OK;
}

extern "C" int st3d_vgg_set_conv(st3d_vgg *vgg, int module_idx, const float *w, const float *b, st3d_stream_t stream) {
    ST3D_CHECK_ARG(vgg && w && b);
    const int s = conv_slot(module_idx);
    ST3D_CHECK_ARG(s >= 0);
    ++vgg->sets;            // (first: a call that fails half way has changed the packs too)
    ST3D_TRY(st3d_conv3x3_pack(w, kConvCout[s], kConvCin[s], vgg->wf[s], vgg->wd[s], stream));
    if (vgg->uf[s]) ST3D_TRY(st3d_wino_pack(w, kConvCout[s], kConvCin[s], vgg->uf[s], vgg->ud[s], stream));
    if (vgg->u6f[s]) ST3D_TRY(st3d_wino43_pack(w, kConvCout[s], kConvCin[s], vgg->u6f[s], vgg->u6d[s], stream));
    ST3D_HIP(hipMemcpyAsync(vgg->bias[s], b, kConvCout[s] * sizeof(float), hipMemcpyDeviceToDevice, st3d::as_stream(stream)));
    vgg->set[s] = true;
    return ST3D_OK;
}

extern "C" int st3d_vgg_destroy(st3d_vgg *vgg) {
    if (!vgg) return ST3D_OK;
    for (int i = 0; i < 16; ++i) {
        if (vgg->wf[i]) (void)hipFree(vgg->wf[i]);
        if (vgg->wd[i]) (void)hipFree(vgg->wd[i]);
        if (vgg->uf[i]) (void)hipFree(vgg->uf[i]);
        if (vgg->ud[i]) (void)hipFree(vgg->ud[i]);
        if (vgg->u6f[i]) (void)hipFree(vgg->u6f[i]);
        if (vgg->u6d[i]) (void)hipFree(vgg->u6d[i]);
        if (vgg->bias[i]) (void)hipFree(vgg->bias[i]);
    }
    delete vgg;
    return ST3D_OK;
}

struct GraphKey {               // what a captured loss step has baked in
    int n = 0, denom = 0;
    bool want_grad = false, masked = false, flat = false;
    float sw = 0.f, cw = 0.f;
    bool guided = false;
    bool operator==(const GraphKey &o) const {
        return n == o.n && denom == o.denom && want_grad == o.want_grad && masked == o.masked && flat == o.flat && sw == o.sw && cw == o.cw &&
               guided == o.guided;
    }
};

struct st3d_plan {
    st3d_vgg *vgg = nullptr;
    int B = 0, S = 0;
    std::vector<void *> owned;      // every device buffer of the plan (dev_alloc); the members below point into these
    size_t bytes = 0;
    // per module: output activation (conv: post-ReLU; relu: alias of its conv; pool: pooled)
    float *act[kModules] = {};
    int C[kModules] = {}, H[kModules] = {}, W[kModules] = {};
    // image i0 of a buffer shaped like module m's output (act[m], the argmax of the pool at m)
    template <typename T> T *at(T *buf, int m, int i0) const { return buf + (size_t)i0 * C[m] * H[m] * W[m]; }
    uint8_t *pidx[5] = {};
    float *gbuf[2] = {};
    size_t gbuf_floats = 0;
    Route route[16];
    // relu1_1 style gradient + ReLU gate + conv1_1 input gradient in one pass (tap0.hip); its 27 tap planes go through the
    // idle gradient buffer
    bool fused_tap0 = false;
    // targets
    float *content_target = nullptr;   // (B, 512, S/8, S/8)
    float *style_gram[5] = {};          // (B or 1, C, C)
    int style_batch = 0;
    bool have_content = false, have_style = false;
    // per-step scratch
    float *gram[5] = {}, *D[5] = {};
    float *gram_ws = nullptr;
    size_t gram_ws_bytes = 0;
    float *partials = nullptr;
    int last_n = 0;
    // profiling
    bool prof = false;
    struct Ev { int fam, module; hipEvent_t a, b; };
    std::vector<Ev> evs;
    std::vector<hipEvent_t> pool;
    float fam_ms[ST3D_PROFILE_FAMILIES] = {};
    int fam_n[ST3D_PROFILE_FAMILIES] = {};
    std::vector<int> l_tag;        // per launch since the last read: family * 100 + VGG module index
    std::vector<float> l_ms;
    // HIP-graph replay of the loss step (st3d_plan_graph): the launch sequence is static, so after one ordinary call
    // (gwarm) it is captured once per key and replayed; it works on plan-owned staging buffers because a captured
    // kernel's pointers are baked in while the caller's tensors move
    int use_graph = 0;
    hipGraphExec_t gexec = nullptr;
    hipStream_t cap_stream = nullptr;
    float *g_in = nullptr, *g_grad = nullptr, *g_loss = nullptr, *g_color = nullptr;
    uint8_t *g_mask = nullptr;
    GraphKey gkey;
    bool gwarm = false;
    // What st3d_plan_create decided about the lists (planlists.h): how many need, flat-field and kept levels, their
    // geometries, the split mode and what a group of a split call walks.  The need lists are rebuilt by every masked call,
    // the flat-field lists by every call that brings a colour, the kept lists once per epoch by its first clean call.
    PlanDecisions d;
    uint8_t *need_flags = nullptr, *flat_ws = nullptr, *keep_ws = nullptr;      // the builders' workspaces
    size_t need_flags_bytes = 0, flat_ws_bytes = 0, keep_ws_bytes = 0;
    // What the list builds write and the launches read: the need lists (segment bytes, tile lists, counts, the Gram run
    // list) and the flat-field lists (tile lists, maps, counts).  sets[0] belongs to the unkeyed calls, which rebuild it
    // every time; sets[1 ..] hold the lists of the last kEpochSlots geometry epochs of st3d_plan_loss_keyed (epochs.h), built
    // once per epoch.  `ls` is the set the launches of the current call read.  A set is need_seg + the lists: 0.6 MB for 8
    // views at 512^2 (st3d_need_blocks_entries, st3d_need_blocks_gram_runs, st3d_flat_tiles) next to the plan's 4.4 GB, so
    // three epochs stay: what a run that alternates two or three view batches needs.
    static constexpr int kEpochSlots = 3;
    // One batch's lists, numbered from its first image: the whole batch of a call, or one group of a split call (below) --
    // the same builders on the group's slice of the coverage.  A group walks its flat_* lists without fills at the shallow
    // levels that have no kept list (they name their representatives within the group; every tile they leave out holds the
    // fill of the epoch's first call, which is what its own launch would write).
    struct Lists {
        uint8_t *need_seg = nullptr;
        int *need_list[ST3D_NEED_MAX_LISTS] = {}, *need_cnt = nullptr;
        int *need_gram_list = nullptr, *need_gram_cnt = nullptr;
        int *kept_list[ST3D_NEED_MAX_LISTS] = {}, *kept_cnt = nullptr;     // (keyed sets) lists keep_first .. of st3d_kept_build
        int *flat_list[3] = {}, *flat_map[3] = {}, *flat_cnt = nullptr;
    };
    struct ListSet {
        Lists whole;
        Lists grp[2];                                   // (keyed sets, split plans)
        uint8_t *c1_skip = nullptr;                     // (keyed sets) conv1_1's tiles that see background only (conv.hip)
        bool have_need = false, have_flat = false;      // (keyed sets) built for the slot's epoch
        bool have_kept = false;                         // (keyed sets) built by the epoch's first clean call
        bool have_grp_fwd = false, have_grp_need = false;       // built by the epoch's first split call, per direction
    };
    ListSet sets[1 + kEpochSlots];
    ListSet *ls = &sets[0];
    st3d::EpochSlots<kEpochSlots> epochs;
    // The clean record: which epoch's background the unlisted tiles of the buffers st3d_flat_fill writes hold -- act[4] and
    // pidx[0] (conv1_2 pooled), act[5] (conv2_1), act[9] and pidx[1] (conv2_2 pooled) -- and with them the background tiles
    // of act[0] (conv1_1).  A keyed call that finds its own epoch, n, colour, level count and weights here launches no
    // fill: its lists are the epoch's, so the listed launches rewrite exactly the tiles they wrote before and the rest still
    // hold what the fills of the epoch's first call copied.  Its conv1_1 likewise leaves out the tiles whose windows see
    // background only (c1_skip): the full launch of the epoch's first call wrote them.
    // The same record vouches for act[10], act[12] and act[14] (conv3_1 .. conv3_3, each a buffer of its own from dev_alloc): a call
    // that sets it ran those launches in full or over their kept lists, so every tile holds what a full launch of that call
    // would have written or -- where the coverage cannot reach -- what the epoch's earlier call did, which is the same bits.
    // The only writer of act[] and pidx[] is forward(), which clears the record on entry; its callers are st3d_plan_forward,
    // st3d_plan_set_content, st3d_plan_set_style and plan_loss_enqueue (every st3d_plan_loss* entry, graph capture and
    // replay included: a replay runs forward()'s captured launches, and the keyed entry never replays).  The backward
    // passes write gbuf[] and the caller's gradient only.  st3d_plan_loss_keyed sets the record after a call whose every
    // launch was enqueued, so a failed call leaves it cleared; st3d_vgg_set_conv changes what a fill would copy and is
    // caught by the handle's counter.
    st3d::CleanRecord clean;
    bool conv1_skip = false;        // conv1_1 of a clean keyed call runs over its covered tiles only (ST3D_FLAT_CONV1=0: in full)
    bool flat_check = false;        // ST3D_FLAT_CHECK=1 (read by st3d_plan_create): keyed calls test their premise on the pixels
    // The split batch (ST3D_SPLIT_BATCH, read by st3d_plan_create): a keyed call that finds the clean record its
    // own runs its n images as two groups of n / 2: the first on the caller's stream, the second on a stream of the plan's.
    // Image i at layer L + 1 reads only image i at layer L, in both directions, so one group's launch can fill the CUs that
    // the other group's launch has left while its last workgroups finish.  The plan's stream is forked from the caller's by
    // an event and joined back by an event before the call returns; the Grams and the loss sums run over the whole batch
    // between the two forks.  (Both groups on streams of the plan's was measured too and loses: each cross-queue dependency
    // leaves the chip idle for 20 - 29 us, and that way there are four per step with nothing running under them; this way
    // the first group's chain starts on the previous launch's end stamp and only the two joins wait.)  A group's slices:
    // images [i0, i0 + n / 2) of act[], pidx[], D[], the targets and the caller's gradient; one fixed half of each gbuf[]
    // (the groups are at different layers at the same time, so a slice by the layer's own image size would overlap).
    // Every launch is per image, tile or block and takes its reduction order from the layer, not from N, so each image
    // gets the bits of the one-stream call (the listed launches by the premise of their lists).
    hipStream_t gstream = nullptr;
    hipEvent_t ev_fork[2] = {}, ev_join[2] = {};    // [forward / backward]
    int split_calls[2] = {};        // calls whose forward / backward ran split (st3d_plan_split_calls)
    // guidance of the style term (st3d_plan_set_style_guidance; guide.hip): the q planes of the five taps for guide_n
    // images (0 = off), and w_0 = q_0^2 for the fused bottom pass.  Allocated by the first call that sets a guidance (for B
    // images: the pointers never move, so a captured loss step keeps reading them), rebuilt by every such call.
    int guide_n = 0;
    float *guide_q = nullptr, *guide_w0 = nullptr, *guide_sums = nullptr, *guide_parts = nullptr;
    const float *guide_plane(int level) const {
        size_t off = 0;
        for (int l = 0; l < level; ++l) off += (size_t)guide_n * (S >> l) * (S >> l);
        return guide_q + off;
    }
};

namespace {

template <typename T>
int dev_alloc(st3d_plan *p, T **ptr, size_t count) {
    const size_t bytes = count * sizeof(T);
    if (hipMalloc(reinterpret_cast<void **>(ptr), bytes) != hipSuccess) {
        st3d::set_error("st3d_plan_create: hipMalloc(%zu bytes) failed", bytes);
        return ST3D_E_NOMEM;
    }
    p->owned.push_back(*ptr);
    p->bytes += bytes;
    // ST3D_POISON_PLAN=1 (tests): the plan's buffers start as 0xFF.. (NaN / -1) instead of whatever hipMalloc returns, so a
    // launch that reads a buffer before the sequence has written it changes the result
    static const bool poison = [] { const char *e = getenv("ST3D_POISON_PLAN"); return e && e[0] == '1'; }();
    if (poison) (void)hipMemset(*ptr, 0xFF, bytes);
    return ST3D_OK;
}

struct Scope {   // HIP-event bracket around one kernel family (only when profiling is on)
    st3d_plan *p; int fam, module; hipStream_t s; hipEvent_t a, b; bool on;
    Scope(st3d_plan *p_, int fam_, hipStream_t s_, int module_ = 99) : p(p_), fam(fam_), module(module_), s(s_), on(p_->prof) {
        if (!on) return;
        auto get = [&]() {
            hipEvent_t e;
            if (!p->pool.empty()) { e = p->pool.back(); p->pool.pop_back(); } else { (void)hipEventCreate(&e); }
            return e;
        };
        a = get(); b = get();
        (void)hipEventRecord(a, s);
    }
    ~Scope() {
        if (!on) return;
        (void)hipEventRecord(b, s);
        p->evs.push_back({fam, module, a, b});
    }
};

// F_CONV_*: the Winograd launches; F_CONVX_*: the convs Winograd does not cover (conv1_1, odd shapes, ST3D_CONV=direct)
// F_CONV43_*: the launches that ran Winograd F(4x4,3x3) (wino43.hip: 2.25 instead of 4 MFMA-multiplies per output)
enum { F_CONV_FWD = 0, F_CONV_DGRAD = 1, F_POOL = 2, F_GRAM_FWD = 3, F_GRAM_BWD = 4, F_ELEM = 5, F_CONVX_FWD = 6, F_CONVX_DGRAD = 7,
       F_CONV43_FWD = 8, F_CONV43_DGRAD = 9,
       // launches that ran over a need list: a fraction of the full launch's work, so not priced as one
       F_CONV43_DGRAD_NEED = 10, F_CONVX_DGRAD_NEED = 11, F_GRAM_BWD_NEED = 12,
       // forward launches over a flat-field list, and the copies that fill in the tiles they left out
       F_CONV43_FWD_FLAT = 13, F_FLAT_FILL = 14,
       // the conv1_1 launch that leaves out its background tiles: a fraction of the full launch's 537 MB write
       F_CONVX_FWD_FLAT = 15 };
static_assert(F_CONVX_FWD_FLAT + 1 == ST3D_PROFILE_FAMILIES, "profile families");

// keep_full: also materialise the full-resolution output of convs whose 2x2 pool is fused into
// their epilogue (needed only when a caller asks for that activation: st3d_plan_forward).
// flat_color (device, 3 floats; the loss call only): imgs hold this colour at many pixels -- conv slots 1 .. 3 (conv1_2,
// conv2_1, conv2_2) compute the tiles of their flat-field lists and copy the rest (flat.hip); the buffers end up bitwise
// what the full launches write
// key (st3d_plan_loss_keyed; p->ls is the epoch's list set): the flat-field lists come from the coverage and are built only
// if the set does not hold them yet, and the fills are left out while the clean record says the buffers hold this epoch's
// background already
struct Keyed {
    uint64_t epoch;
    const uint8_t *cover;       // (n,S,S) device bytes, non-zero = covered; every other pixel holds the colour bit for bit
    const float *rgb;           // the colour again, 3 floats in HOST memory (what the clean record compares)
    int flat_done;              // out: how many launches ran listed
    int kept_done;              // out: how many of conv3_1 .. conv3_3 the call leaves whole (in full or over their kept lists)
    bool clean_call = false;    // out: the call found the clean record its own (no fill ran; what a split call requires)
};
// the lists a forward chain walks: the epoch's whole-batch ones, or one group's (split calls)
struct FwdLists {
    const st3d_plan::Lists &lists;
    const uint8_t *c1_skip;     // the chain's first image's slice of the set's (nullptr: none)
    const bool *kept_on;        // (groups) which kept lists the group walks; nullptr = all the plan has
};

// may this call run as two groups in direction `dir`?  (what the call itself decides -- a clean record, a mask -- is the caller's)
bool split_ok(const st3d_plan *p, int dir, int n, bool keyed) {
    return keyed && (p->d.split_mode & dir) && p->gstream && !p->prof && !p->use_graph && p->guide_n == 0 && n >= 4 && n % 2 == 0;
}
// join the plan's stream back into s (dir: 0 the forward's event, 1 the backward's)
int split_join(st3d_plan *p, int dir, hipStream_t s) {
    ST3D_HIP(hipEventRecord(p->ev_join[dir], p->gstream));
    ST3D_HIP(hipStreamWaitEvent(s, p->ev_join[dir], 0));
    return ST3D_OK;
}
// A split call's chain: fork the plan's stream from s, then fn(g, stream) for the first group on s and the second on the
// plan's stream, stopping at the first failure.  The plan's stream is joined back also after a failure (the caller's stream
// stays behind whatever was enqueued).  -> the first error; split_calls[dir] counts the calls that went through.
// (dir: 0 the forward's events and count, 1 the backward's)
template <typename Fn>
int run_split(st3d_plan *p, int dir, hipStream_t s, Fn fn) {
    ST3D_HIP(hipEventRecord(p->ev_fork[dir], s));
    ST3D_HIP(hipStreamWaitEvent(p->gstream, p->ev_fork[dir], 0));
    int rc = ST3D_OK;
    for (int g = 0; g < 2 && rc == ST3D_OK; ++g) rc = fn(g, g == 0 ? s : p->gstream);
    const int rj = split_join(p, dir, s);
    if (rc != ST3D_OK || rj != ST3D_OK) return rc != ST3D_OK ? rc : rj;
    ++p->split_calls[dir];
    return ST3D_OK;
}

// The lists a keyed call's forward walks, from the coverage of `images` images (the batch, or one group's slice): the
// flat-field lists (with the set's c1_skip bytes when given) and the kept lists, each when asked for.
int build_forward_lists(st3d_plan *p, st3d_plan::Lists &L, const uint8_t *cover, int images, int flat, bool want_flat, uint8_t *c1_skip,
                        bool want_kept, hipStream_t s) {
    if (want_flat) {
        Scope sc(p, F_ELEM, s);
        ST3D_TRY(st3d_flat_build_cover(cover, images, p->S, flat, p->flat_ws, p->flat_ws_bytes, L.flat_list[0], L.flat_map[0], L.flat_list[1],
                                       L.flat_map[1], L.flat_list[2], L.flat_map[2], L.flat_cnt, s));
        if (c1_skip) ST3D_TRY(st3d_conv1_skip_build(cover, images, p->S, p->S, c1_skip, s));
    }
    if (want_kept) {
        Scope sc(p, F_ELEM, s);
        ST3D_TRY(st3d_kept_build(cover, images, p->S, p->d.keep_first, kKeepFirst + p->d.keep_levels, p->d.keep_cols, p->keep_ws,
                                 p->keep_ws_bytes, L.kept_list, L.kept_cnt, s));
    }
    return ST3D_OK;
}

// The need lists of `need` levels from the mask of `images` images (the batch, or one group's slice): the per-block ones
// (gram: with the relu2_1 run list), or the tile-granular ones where the plan has no others or a single level asks for none.
int build_need_lists(st3d_plan *p, st3d_plan::Lists &L, const uint8_t *mask, int images, int need, bool gram, hipStream_t s) {
    Scope sc(p, F_ELEM, s);
    if (p->d.need_blocks && need >= 2)
        return st3d_need_blocks_build(mask, images, p->S, need - 1, p->d.need_cols, L.need_seg, p->need_flags, p->need_flags_bytes, L.need_list,
                                      L.need_cnt, gram ? L.need_gram_list : nullptr, L.need_gram_cnt, s);
    return st3d_need_build(mask, images, p->S, need, L.need_seg, p->need_flags, p->need_flags_bytes, L.need_list[0], L.need_list[1], L.need_cnt, s);
}

// conv slot cs of a clean keyed call over its kept list, in strips (cols = 16) or tiles; yp, yi: the fused pool's outputs
// (tiles only) or nullptr.  The tiles it leaves out hold the previous call's bits.
int kept_launch(st3d_plan *p, int cs, const float *x, float *y, float *yp, uint8_t *yi, int n, int cols, const st3d_plan::Lists &L,
                hipStream_t s) {
    const st3d_vgg *v = p->vgg;
    const int m = kConvIdx[cs], k = cs - 1, Cin = kConvCin[cs], Cout = kConvCout[cs], H = p->H[m], W = p->W[m];
    Scope sc(p, F_CONV43_FWD_FLAT, s, m);
    if (cols == 16) return st3d_wino43_fwd_strips(x, v->u6f[cs], v->bias[cs], y, n, Cin, Cout, H, W, 1, L.kept_list[k], L.kept_cnt + k, s);
    return st3d_wino43_fwd_tiles_geo(x, v->u6f[cs], v->bias[cs], y, yp, yi, n, Cin, Cout, H, W, 1, cols, L.kept_list[k], L.kept_cnt + k, s);
}

// the launches of images [i0, i0 + n) from module 0 to upto on stream s; x: the first of those images
int forward_chain(st3d_plan *p, const float *x, int i0, int n, int upto, bool keep_full, hipStream_t s, int flat, int keep, bool fill,
                  const FwdLists &fl) {
    const st3d_vgg *v = p->vgg;
    const st3d_plan::Lists &L = fl.lists;
    auto act = [&](int m) { return p->at(p->act[m], m, i0); };
    auto on = [&](int k) { return !fl.kept_on || fl.kept_on[k]; };
    for (int m = 0; m <= upto; ++m) {
        const int cs = conv_slot(m), ps = pool_slot(m);
        if (cs >= 0) {
            if (!v->set[cs]) {
                st3d::set_error("st3d_plan_forward: weights of module %d were never set", m);
                return ST3D_E_STATE;
            }
            const int Cin = kConvCin[cs], Cout = kConvCout[cs], H = p->H[m], W = p->W[m];
            const uint8_t route = p->route[cs].fwd;
            if (route == DIRECT && cs == 0 && !fill && fl.c1_skip) {     // conv1_1 of a clean keyed call: the covered tiles
                Scope sc(p, F_CONVX_FWD_FLAT, s, m);
                ST3D_TRY(st3d_conv3x3_fwd_skip(x, v->wf[cs], v->bias[cs], act(m), n, Cin, Cout, H, W, 1, fl.c1_skip, s));
                x = act(m);
                continue;
            }
            if (route == DIRECT) {
                Scope sc(p, F_CONVX_FWD, s, m);
                ST3D_TRY(st3d_conv3x3_fwd(x, v->wf[cs], v->bias[cs], act(m), n, Cin, Cout, H, W, 1, s));
                x = act(m);
                continue;
            }
            // the Winograd kernels pool in their epilogue: conv, relu and the pool behind them are one launch
            const int pool_m = m + 2;
            const int pps = (pool_m <= upto) ? pool_slot(pool_m) : -1;
            float *yfull = (pps < 0 || keep_full) ? act(m) : nullptr;
            float *yp = pps >= 0 ? act(pool_m) : nullptr;
            uint8_t *yi = pps >= 0 ? p->at(p->pidx[pps], pool_m, i0) : nullptr;
            // a clean keyed call: the geometry of the kept list this launch walks (0: none) -- a shallow level's own, or the
            // tiles of conv3_1 .. that the coverage can change (no pool there: yfull is the output, yp and yi are null)
            // (the range first: only conv slots 1 .. flat and kKeepFirst + 1 .. kKeepFirst + keep name a list)
            const bool listed = cs >= 1 && (cs <= flat || (cs > kKeepFirst && cs <= kKeepFirst + keep));
            const int kept_cols = !(listed && !fill && keep > 0 && on(cs - 1)) ? 0 : cs <= flat ? p->d.shallow_cols[cs - 1] : p->d.keep_cols[cs - 1];
            if (kept_cols) {
                ST3D_TRY(kept_launch(p, cs, x, yfull, yp, yi, n, kept_cols, L, s));
            } else if (cs >= 1 && cs <= flat) {    // an F(4x4,3x3) launch over its flat-field list, then the copies
                {
                    Scope sc(p, F_CONV43_FWD_FLAT, s, m);
                    ST3D_TRY(st3d_wino43_fwd_tiles(x, v->u6f[cs], v->bias[cs], yfull, yp, yi, n, Cin, Cout, H, W, 1, L.flat_list[cs - 1],
                                                   L.flat_cnt + (cs - 1), s));
                }
                if (fill) {
                    Scope sc(p, F_FLAT_FILL, s, m);
                    ST3D_TRY(st3d_flat_fill(L.flat_map[cs - 1], yfull, yp, yi, n, Cout, H, W, s));
                }
            } else if (route == WINO43) {
                Scope sc(p, F_CONV43_FWD, s, m);
                ST3D_TRY(st3d_wino43_fwd(x, v->u6f[cs], v->bias[cs], yfull, yp, yi, n, Cin, Cout, H, W, 1, s));
            } else {
                Scope sc(p, F_CONV_FWD, s, m);
                ST3D_TRY(st3d_wino_fwd(x, v->uf[cs], v->bias[cs], yfull, yp, yi, n, Cin, Cout, H, W, 1, s));
            }
            x = pps >= 0 ? yp : act(m);
            if (pps >= 0) m = pool_m;               // modules m+1, m+2 are done
        } else if (ps >= 0) {                       // (the ReLU before it kept its conv's C, H, W)
            Scope sc(p, F_POOL, s, m);
            ST3D_TRY(st3d_maxpool2x2_fwd(x, act(m), p->at(p->pidx[ps], m, i0), n, p->C[m], p->H[m - 1], p->W[m - 1], s));
            x = act(m);
        }   // ReLU modules are fused into their conv
    }
    return ST3D_OK;
}

int forward(st3d_plan *p, const float *imgs, int n, int upto, bool keep_full, hipStream_t s, const float *flat_color = nullptr,
            Keyed *key = nullptr) {
    const st3d_vgg *v = p->vgg;
    st3d_plan::ListSet *ls = p->ls;
    int flat = 0;               // conv slots 1 .. flat run listed
    if (flat_color)
        while (flat < p->d.flat_levels && kConvIdx[flat + 1] <= upto) ++flat;
    int keep = 0;               // conv slots 4 .. 3 + keep (conv3_1 ..) may run over their kept lists
    if (key && flat == p->d.flat_levels)
        while (keep < p->d.keep_levels && kConvIdx[kKeepFirst + 1 + keep] <= upto) ++keep;
    const bool fill = !(key && flat > 0 && p->clean.matches(key->epoch, n, flat, key->rgb, v->sets, keep));
    p->clean.clear();           // every path below writes act[] / pidx[]; the keyed entry sets the record again when all went well
    if (flat > 0 && !key) {
        Scope sc(p, F_ELEM, s);
        st3d_plan::Lists &L = ls->whole;
        ST3D_TRY(st3d_flat_build(imgs, flat_color, n, p->S, flat, p->flat_ws, p->flat_ws_bytes, L.flat_list[0], L.flat_map[0], L.flat_list[1],
                                 L.flat_map[1], L.flat_list[2], L.flat_map[2], L.flat_cnt, s));
    } else if (flat > 0 && p->flat_check) {     // the premise on this call's pixels: one host read, debug runs only
        int bad = 0, *cnt = p->sets[0].whole.flat_cnt + 3;
        ST3D_TRY(st3d_flat_check_cover(imgs, flat_color, key->cover, n, p->S, p->flat_ws, p->flat_ws_bytes, cnt, s));
        ST3D_HIP(hipMemcpyAsync(&bad, cnt, sizeof(int), hipMemcpyDeviceToHost, s));
        ST3D_HIP(hipStreamSynchronize(s));
        if (bad) {
            st3d::set_error("st3d_plan_loss_keyed: a pixel outside the coverage differs from the background colour");
            return ST3D_E_STATE;
        }
    }
    if (key) {
        // the flat-field lists once per epoch; the kept lists by the epoch's first clean call (a run that changes its
        // geometry every step never gets there).  Each flag is set as soon as its build is enqueued.
        const bool want_flat = flat > 0 && !ls->have_flat, want_kept = !fill && keep > 0 && !ls->have_kept;
        ST3D_TRY(build_forward_lists(p, ls->whole, key->cover, n, flat, want_flat, ls->c1_skip, false, s));
        ls->have_flat |= want_flat;
        key->flat_done = flat; key->kept_done = keep; key->clean_call = !fill;
        ST3D_TRY(build_forward_lists(p, ls->whole, key->cover, n, flat, false, nullptr, want_kept, s));
        ls->have_kept |= want_kept;
    }
    if (!fill && upto == 28 && !keep_full && split_ok(p, SPLIT_FWD, n, key != nullptr)) {
        // ---- the clean call as two groups; the epoch's first split call runs the builders once more, on each group's slice
        const int h = n / 2;
        for (int g = 0; g < 2 && !ls->have_grp_fwd; ++g)
            ST3D_TRY(build_forward_lists(p, ls->grp[g], key->cover + (size_t)g * h * p->S * p->S, h, flat, true, nullptr, keep > 0, s));
        ls->have_grp_fwd = true;
        ST3D_TRY(run_split(p, 0, s, [&](int g, hipStream_t gs) {
            const FwdLists fl{ls->grp[g], ls->c1_skip ? ls->c1_skip + st3d_conv1_skip_tiles(1, p->S, p->S) * (size_t)g * h : nullptr,
                              p->d.grp_kept_on};
            return forward_chain(p, imgs + (size_t)g * h * 3 * p->S * p->S, g * h, h, upto, keep_full, gs, flat, keep, fill, fl);
        }));
    } else {
        ST3D_TRY(forward_chain(p, imgs, 0, n, upto, keep_full, s, flat, keep, fill, FwdLists{ls->whole, ls->c1_skip, nullptr}));
    }
    p->last_n = n;
    return ST3D_OK;
}

// w = q * q (the weight plane of the fused bottom pass from the q plane of level 0)
__global__ __launch_bounds__(256) void square_kernel(const float *__restrict__ q, size_t n, float *__restrict__ w) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) w[i] = q[i] * q[i];
}

// g = (accumulate ? g : 0) + x
__global__ __launch_bounds__(256) void add_kernel(const float *__restrict__ x, size_t n, int accumulate, float *__restrict__ g) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) g[i] = accumulate ? g[i] + x[i] : x[i];
}

// backward of MaxPool2d(2,2) as a stand-alone pass: out (planes,H,W) = scatter of gp (planes,H/2,W/2) to the argmax
// positions (+ `add`, a full-resolution gradient arriving at the same tensor, when given).  Only the differentiable
// get_features needs it (a tap on a conv that feeds a pool); the loss plan fuses the unpool into the dgrad kernel.
__global__ __launch_bounds__(256) void unpool_add_kernel(const float *__restrict__ gp, const uint8_t *__restrict__ idx,
                                                         const float *__restrict__ add, size_t planes, int H, int W,
                                                         float *__restrict__ out) {
    const int Hp = H / 2, Wp = W / 2;
    const size_t n = planes * (size_t)Hp * Wp;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int xo = (int)(i % Wp), yo = (int)((i / Wp) % Hp);
    const size_t pl = i / ((size_t)Wp * Hp);
    const float g = gp ? gp[i] : 0.f;
    const int k = gp ? idx[i] : -1;
    const size_t base = pl * H * W + (size_t)(2 * yo) * W + 2 * xo;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const size_t o = base + (size_t)(q >> 1) * W + (q & 1);
        out[o] = (q == k ? g : 0.f) + (add ? add[o] : 0.f);
    }
}

// what the loss plan's chain adds to a plain input-gradient launch
struct DgradOpts {
    bool pregated = false;              // g is already zero where the gate this launch would apply is closed
    const float *out_gate = nullptr;    // zero dst where this tensor is <= 0 (the next link's gate, Winograd only)
    const float *add_target = nullptr;  // dst += add_coef * (out_gate - add_target): the content term, joining in the store
    float add_coef = 0.f;
    // compute the listed output tiles only (F(4x4,3x3) launches; anything else is an error, not a silent full launch: the
    // caller has already skipped the work above on the strength of it)
    const int *tile_list = nullptr, *n_active = nullptr;
    int tile_cols = 0;                  // the geometry the list numbers (0 = st3d_wino43_tile_geometry's)
};

// one input-gradient launch of conv slot cs: g (gradient w.r.t. the conv's post-ReLU output, or w.r.t. the output of
// the pool behind it when pooled) -> dst (gradient w.r.t. the conv's input)
// (i0: the first image of g and dst in the plan's buffers -- the gates, pooled values and argmax are read from there on)
int dgrad_step(st3d_plan *p, int cs, const float *g, bool g_is_pooled, int pool_of_g, float *dst, int n, hipStream_t s,
               const DgradOpts &o = {}, int i0 = 0) {
    const st3d_vgg *v = p->vgg;
    const int m = kConvIdx[cs];
    const int Cin = kConvCin[cs], Cout = kConvCout[cs], H = p->H[m], W = p->W[m];
    const bool wino = p->route[cs].dgrad_wino;
    const bool w43 = p->route[cs].dgrad_w43 && o.pregated;
    if (o.tile_list && !w43) {
        st3d::set_error("st3d_plan_loss_masked: the input gradient of module %d is not an F(4x4,3x3) launch", m);
        return ST3D_E_STATE;
    }
    Scope sc(p, o.tile_list ? F_CONV43_DGRAD_NEED : w43 ? F_CONV43_DGRAD : (wino ? F_CONV_DGRAD : F_CONVX_DGRAD), s, m);
    const int pm = g_is_pooled ? kPoolIdx[pool_of_g] : 0;
    const uint8_t *pidx = g_is_pooled ? p->at(p->pidx[pool_of_g], pm, i0) : nullptr;
    const float *pooled = g_is_pooled ? p->at(p->act[pm], pm, i0) : nullptr;
    const float *act_m = p->at(p->act[m], m, i0);
    if (o.tile_list)
        ST3D_TRY(st3d_wino43_dgrad_chain_tiles_geo(g, pidx, v->u6d[cs], o.out_gate, o.add_target, o.add_coef, dst, n, Cin, Cout, H, W,
                                                   o.tile_cols, o.tile_list, o.n_active, s));
    else if (w43)
        ST3D_TRY(st3d_wino43_dgrad_chain(g, pidx, v->u6d[cs], o.out_gate, o.add_target, o.add_coef, dst, n, Cin, Cout, H, W, s));
    else if (wino && (o.pregated || o.out_gate))
        ST3D_TRY(st3d_wino_dgrad_chain(g, (g_is_pooled || o.pregated) ? nullptr : act_m, pidx, o.pregated ? nullptr : pooled,
                                       v->ud[cs], o.out_gate, o.add_target, o.add_coef, dst, n, Cin, Cout, H, W, s));
    else if (g_is_pooled && wino)
        ST3D_TRY(st3d_wino_dgrad_unpool(g, pidx, pooled, v->ud[cs], dst, n, Cin, Cout, H, W, s));
    else if (g_is_pooled)
        ST3D_TRY(st3d_conv3x3_dgrad_unpool(g, pidx, pooled, v->wd[cs], dst, n, Cin, Cout, H, W, s));
    else if (wino)
        ST3D_TRY(st3d_wino_dgrad(g, act_m, v->ud[cs], dst, n, Cin, Cout, H, W, s));
    else
        ST3D_TRY(st3d_conv3x3_dgrad(g, act_m, v->wd[cs], dst, n, Cin, Cout, H, W, s));
    return ST3D_OK;
}

}  // namespace

extern "C" int st3d_plan_create(st3d_plan **out, st3d_vgg *vgg, int B, int S) {
    ST3D_CHECK_ARG(out && vgg);
    ST3D_CHECK_ARG(B > 0 && S >= 16);      // any size: shapes the Winograd kernels do not cover (odd H, W % 4) run on the direct ones, pools floor like MaxPool2d
    st3d_plan *p = new st3d_plan();
    p->vgg = vgg; p->B = B; p->S = S;
    int rc = ST3D_OK;
    auto alloc = [&](auto **ptr, size_t count) { if (rc == ST3D_OK) rc = dev_alloc(p, ptr, count); };
    size_t gmax = 0, wsmax = 0;
    for (int m = 0, C = 3, H = S, W = S; m < kModules; ++m) {
        const int cs = conv_slot(m), ps = pool_slot(m);
        if (cs >= 0) {
            C = kConvCout[cs];
            alloc(&p->act[m], (size_t)B * C * H * W);
            if ((size_t)B * C * H * W > gmax) gmax = (size_t)B * C * H * W;
        } else if (ps >= 0) {
            H /= 2; W /= 2;
            alloc(&p->act[m], (size_t)B * C * H * W);
            alloc(&p->pidx[ps], (size_t)B * C * H * W);
        } else {
            p->act[m] = p->act[m - 1];   // in-place ReLU: the tap tensor IS the post-ReLU output
        }
        p->C[m] = C; p->H[m] = H; p->W[m] = W;
    }
    p->gbuf_floats = gmax;
    // ---- the route table and what follows from it: the one place that reads the handle's switches and asks the kernels
    // what they cover
    const st3d_vgg *v = vgg;
    for (int cs = 0; cs < 16 && v->use_wino; ++cs) {
        const int m = kConvIdx[cs], Cin = kConvCin[cs], Cout = kConvCout[cs], H = p->H[m], W = p->W[m];
        // F(4x4,3x3) for a GEMM that reduces over K channels (Cin forward, Cout for the input gradient) and produces M
        auto w43 = [&](int K, int M) { return v->wino43_mink > 0 && v->u6f[cs] && K >= v->wino43_mink && st3d_wino43_supported(K, M, H, W); };
        Route &r = p->route[cs];
        if (v->uf[cs] && st3d_wino_supported(Cin, Cout, H, W)) r.fwd = w43(Cin, Cout) ? WINO43 : WINO;
        r.dgrad_wino = v->ud[cs] && st3d_wino_supported(Cout, Cin, H, W);
        r.dgrad_w43 = r.dgrad_wino && w43(Cout, Cin);
        r.gate_taps = v->pregate && r.dgrad_wino && (Cout % 32) == 0;       // (what the gated tap kernels take)
        r.gate_dst = v->pregate && cs > 0 && r.dgrad_wino && p->route[cs - 1].dgrad_wino;
    }
    p->fused_tap0 = v->fuse_tap0 && st3d_conv1_bwd_supported(S, S) && gmax >= (size_t)B * 27 * S * S;
    // ---- what the lists' decisions rest on (planlists.h), asked once: the CU count and the kernels' answers
    PlanFacts f;
    f.B = B; f.S = S;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&f.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || f.cus <= 0) f.cus = 256;
    for (int cs = 0; cs < 16; ++cs) { f.H[cs] = p->H[kConvIdx[cs]]; f.route[cs] = p->route[cs]; }
    f.fused_tap0 = p->fused_tap0;
    f.need_levels = st3d_need_levels(S);
    f.blocks_lists = st3d_need_blocks_lists(S);
    f.flat_levels = st3d_flat_levels(S);
    for (int k = 0; k < ST3D_NEED_MAX_LISTS; ++k) st3d_wino43_tile_geometry(f.H[k + 1], f.H[k + 1], &f.geo_rows[k], &f.geo_cols[k]);
    f.gram_segs = st3d_gram_bwd_segs_supported(p->C[kConvIdx[2]], f.H[2] * f.H[2]) != 0;
    f.gram_runs = st3d_need_blocks_gram_runs(B, S);
    p->d = decide_lists(f, [](const char *name) -> const char * { return getenv(name); });
    const PlanDecisions &d = p->d;
    for (int i = 0; i < 2; ++i) alloc(&p->gbuf[i], gmax);
    alloc(&p->content_target, (size_t)B * p->C[kContentTap] * p->H[kContentTap] * p->W[kContentTap]);
    for (int i = 0; i < 5; ++i) {
        const int m = kStyleTap[i];
        const size_t cc = (size_t)B * p->C[m] * p->C[m];
        alloc(&p->style_gram[i], cc);
        alloc(&p->gram[i], cc);
        alloc(&p->D[i], cc);
    }
    // every style layer has its own split-K slab region: the five Grams of a step run as ONE launch (st3d_gram_fwd_multi).
    // Sized for the worst batch 1..B (the split count is rounded per batch size, so n < B can need a little more than B).
    for (int n = 1; n <= B; ++n) {
        st3d_gram_item items[5];
        for (int i = 0; i < 5; ++i) items[i] = st3d_gram_item{nullptr, nullptr, n, p->C[kStyleTap[i]], p->H[kStyleTap[i]] * p->W[kStyleTap[i]]};
        const size_t ws = st3d_gram_multi_workspace_bytes(items, 5);
        if (ws > wsmax) wsmax = ws;
    }
    p->gram_ws_bytes = wsmax;
    alloc(&p->gram_ws, wsmax / sizeof(float));
    alloc(&p->partials, (size_t)8 * st3d_reduce_partials());
    alloc(&p->g_in, (size_t)B * 3 * S * S);
    alloc(&p->g_grad, (size_t)B * 3 * S * S);
    alloc(&p->g_loss, (size_t)4);
    if (d.need_levels >= 1) {
        alloc(&p->g_mask, (size_t)B * S * S);
        p->need_flags_bytes = d.need_blocks ? st3d_need_blocks_workspace_bytes(B, S) : st3d_need_workspace_bytes(B, S);
        if (d.need_levels >= 2) alloc(&p->need_flags, p->need_flags_bytes);
    }
    if (d.flat_levels >= 1) {
        p->flat_ws_bytes = st3d_flat_workspace_bytes(B, S);
        alloc(&p->flat_ws, p->flat_ws_bytes);
        alloc(&p->g_color, (size_t)4);
    }
    if (d.keep_levels >= 1) {
        p->keep_ws_bytes = st3d_need_blocks_workspace_bytes(B, S);
        alloc(&p->keep_ws, p->keep_ws_bytes);
    }
    // the lists of `images` images: the flat-field ones always, the need and kept ones where the caller says
    auto alloc_lists = [&](st3d_plan::Lists &L, int images, bool need, bool kept) {
        if (need) {
            alloc(&L.need_seg, (size_t)images * S * (S / 64));
            alloc(&L.need_cnt, (size_t)ST3D_NEED_MAX_LISTS);
            if (d.need_gram) {
                alloc(&L.need_gram_list, st3d_need_blocks_gram_runs(images, S));
                alloc(&L.need_gram_cnt, (size_t)1);
            }
            for (int l = 0; l + 2 <= d.need_levels; ++l) {
                if (d.need_blocks) {
                    alloc(&L.need_list[l], st3d_need_blocks_entries(images, S, l, d.need_cols[l]));
                    continue;
                }
                int rows = 0, cols = 0;
                st3d_wino43_tile_geometry(S >> l, S >> l, &rows, &cols);
                alloc(&L.need_list[l], (size_t)images * ((S >> l) / rows) * ((S >> l) / cols));
            }
        }
        if (d.flat_levels >= 1) {
            alloc(&L.flat_cnt, (size_t)4);
            for (int k = 0; k < d.flat_levels; ++k) {
                alloc(&L.flat_list[k], (size_t)st3d_flat_tiles(images, S, k));
                alloc(&L.flat_map[k], (size_t)st3d_flat_tiles(images, S, k));
            }
        }
        if (kept) {
            alloc(&L.kept_cnt, (size_t)ST3D_NEED_MAX_LISTS);
            for (int k = d.keep_first; k < kKeepFirst + d.keep_levels; ++k)
                alloc(&L.kept_list[k], st3d_need_blocks_entries(images, S, k, d.keep_cols[k]));
        }
    };
    if (d.split_mode && rc == ST3D_OK) {
        bool ok = hipStreamCreateWithFlags(&p->gstream, hipStreamNonBlocking) == hipSuccess;
        for (int dir = 0; dir < 2; ++dir)
            ok = ok && hipEventCreateWithFlags(&p->ev_fork[dir], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&p->ev_join[dir], hipEventDisableTiming) == hipSuccess;
        if (!ok) { st3d::set_error("st3d_plan_create: the split batch's stream and events could not be made"); rc = ST3D_E_HIP; }
    }
    auto flag = [](const char *name, bool dflt) { const char *e = getenv(name); return e && e[0] ? e[0] != '0' : dflt; };
    p->flat_check = flag("ST3D_FLAT_CHECK", false);
    p->conv1_skip = d.flat_levels >= 1 && p->route[0].fwd == DIRECT && flag("ST3D_FLAT_CONV1", true);
    // the unkeyed set has the need and flat-field lists of the batch; an epoch's set also its kept lists, conv1_1's skip
    // bytes and, in a split plan, each group's lists (their need lists only the per-block ones: a group's backward requires them)
    for (int i = 0; i <= st3d_plan::kEpochSlots; ++i) {
        st3d_plan::ListSet &ls = p->sets[i];
        alloc_lists(ls.whole, B, d.need_levels >= 1, i >= 1 && d.keep_levels >= 1);
        if (i == 0) continue;
        if (d.split_mode)
            for (st3d_plan::Lists &G : ls.grp) alloc_lists(G, B / 2, d.need_levels >= 1 && d.need_blocks, d.keep_levels >= 1);
        if (p->conv1_skip) alloc(&ls.c1_skip, st3d_conv1_skip_tiles(B, S, S));
    }
    if (rc != ST3D_OK) { st3d_plan_destroy(p); return rc; }
    *out = p;
    return ST3D_OK;
}

extern "C" int st3d_plan_destroy(st3d_plan *p) {
    if (!p) return ST3D_OK;
    for (void *b : p->owned) (void)hipFree(b);
    if (p->gexec) (void)hipGraphExecDestroy(p->gexec);
    if (p->cap_stream) (void)hipStreamDestroy(p->cap_stream);
    if (p->gstream) (void)hipStreamDestroy(p->gstream);
    for (int d = 0; d < 2; ++d) {
        if (p->ev_fork[d]) (void)hipEventDestroy(p->ev_fork[d]);
        if (p->ev_join[d]) (void)hipEventDestroy(p->ev_join[d]);
    }
    for (auto &e : p->evs) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto &e : p->pool) (void)hipEventDestroy(e);
    delete p;
    return ST3D_OK;
}

extern "C" size_t st3d_plan_bytes(const st3d_plan *p) { return p ? p->bytes : 0; }

extern "C" int st3d_plan_forward(st3d_plan *p, const float *imgs, int n, int upto_module, st3d_stream_t stream) {
    ST3D_CHECK_ARG(p && imgs);
    ST3D_CHECK_ARG(n > 0 && n <= p->B && upto_module >= 0 && upto_module < kModules);
    st3d::TraceRange tr("vgg_forward");
    return forward(p, imgs, n, upto_module, true, st3d::as_stream(stream));
}

extern "C" int st3d_plan_activation(st3d_plan *p, int module_idx, float **ptr, int *C, int *H, int *W) {
    ST3D_CHECK_ARG(p && ptr && module_idx >= 0 && module_idx < kModules);
    *ptr = p->act[module_idx];
    if (C) *C = p->C[module_idx];
    if (H) *H = p->H[module_idx];
    if (W) *W = p->W[module_idx];
    return ST3D_OK;
}

extern "C" int st3d_plan_set_content(st3d_plan *p, const float *content, int n, st3d_stream_t stream) {
    ST3D_CHECK_ARG(p && content && n > 0 && n <= p->B);
    hipStream_t s = st3d::as_stream(stream);
    ST3D_TRY(forward(p, content, n, kContentTap, false, s));
    const size_t cnt = (size_t)n * p->C[kContentTap] * p->H[kContentTap] * p->W[kContentTap];
    ST3D_HIP(hipMemcpyAsync(p->content_target, p->act[kContentTap], cnt * sizeof(float), hipMemcpyDeviceToDevice, s));
    p->have_content = true;
    return ST3D_OK;
}

// content features (conv4_2 of the content images) out of / into the plan: lets a caller that alternates between several
// view batches keep each batch's target and skip recomputing it (a device copy instead of a VGG forward to conv4_2)
extern "C" int st3d_plan_get_content_features(st3d_plan *p, float *out, int n, st3d_stream_t stream) {
    ST3D_CHECK_ARG(p && out && n > 0 && n <= p->B);
    if (!p->have_content) {
        st3d::set_error("st3d_plan_get_content_features: no content target set");
        return ST3D_E_STATE;
    }
    const size_t cnt = (size_t)n * p->C[kContentTap] * p->H[kContentTap] * p->W[kContentTap];
    ST3D_HIP(hipMemcpyAsync(out, p->content_target, cnt * sizeof(float), hipMemcpyDeviceToDevice, st3d::as_stream(stream)));
    return ST3D_OK;
}

extern "C" int st3d_plan_set_content_features(st3d_plan *p, const float *feat, int n, st3d_stream_t stream) {
    ST3D_CHECK_ARG(p && feat && n > 0 && n <= p->B);
    const size_t cnt = (size_t)n * p->C[kContentTap] * p->H[kContentTap] * p->W[kContentTap];
    ST3D_HIP(hipMemcpyAsync(p->content_target, feat, cnt * sizeof(float), hipMemcpyDeviceToDevice, st3d::as_stream(stream)));
    p->have_content = true;
    return ST3D_OK;
}

// the five style taps' Grams (of the n images of the last forward) in one launch pair
// (guided: the guided Grams, under the plan's guidance planes)
static int grams_of_taps(st3d_plan *p, int n, float *const *out, hipStream_t s, bool guided = false) {
    st3d_gram_item items[5];
    const float *q[5];
    for (int i = 0; i < 5; ++i) {
        const int m = kStyleTap[i];
        items[i] = st3d_gram_item{p->act[m], out[i], n, p->C[m], p->H[m] * p->W[m]};
        q[i] = guided ? p->guide_plane(i) : nullptr;
    }
    if (guided) return st3d_gram_fwd_multi_weighted(items, q, 5, p->gram_ws, p->gram_ws_bytes, s);
    return st3d_gram_fwd_multi(items, 5, p->gram_ws, p->gram_ws_bytes, s);
}

// Guidance of the style term: mask (n,1,S,S) in [0,1] -> the plan's q planes (st3d_guidance_build); every later
// st3d_plan_loss* call with the same n takes the Gram of each tap over the guided region (the style targets stay the plain
// Grams, the content term is unchanged, the guidance carries no gradient).  mask NULL clears (n is ignored).
extern "C" int st3d_plan_set_style_guidance(st3d_plan *p, const float *mask, int n, st3d_stream_t stream) {
    ST3D_CHECK_ARG(p);
    if (!mask) { p->guide_n = 0; return ST3D_OK; }
    ST3D_CHECK_ARG(n > 0 && n <= p->B);
    hipStream_t s = st3d::as_stream(stream);
    p->guide_n = 0;
    // each buffer once: a call that follows a failed allocation asks only for what is still missing
    if (!p->guide_q) ST3D_TRY(dev_alloc(p, &p->guide_q, st3d_guidance_floats(p->B, p->S)));
    if (!p->guide_w0) ST3D_TRY(dev_alloc(p, &p->guide_w0, (size_t)p->B * p->S * p->S));
    if (!p->guide_sums) ST3D_TRY(dev_alloc(p, &p->guide_sums, (size_t)5 * p->B));
    if (!p->guide_parts) ST3D_TRY(dev_alloc(p, &p->guide_parts, st3d_guidance_partials(p->B, p->S)));
    ST3D_TRY(st3d_guidance_build(mask, n, p->S, p->guide_q, p->guide_sums, p->guide_parts, s));
    const size_t cnt = (size_t)n * p->S * p->S;
    square_kernel<<<(unsigned)std::min<size_t>((cnt + 255) / 256, 65535), 256, 0, s>>>(p->guide_q, cnt, p->guide_w0);
    ST3D_LAUNCH_CHECK();
    p->guide_n = n;
    return ST3D_OK;
}

extern "C" int st3d_plan_set_style(st3d_plan *p, const float *style, int style_batch, int n, st3d_stream_t stream) {
    ST3D_CHECK_ARG(p && style && n > 0 && n <= p->B && (style_batch == 1 || style_batch == n));
    hipStream_t s = st3d::as_stream(stream);
    ST3D_TRY(forward(p, style, style_batch, 28, false, s));
    {
        Scope sc(p, F_GRAM_FWD, s);
        ST3D_TRY(grams_of_taps(p, style_batch, p->style_gram, s));
    }
    if (p->style_batch != style_batch && p->gexec) {       // a captured loss step indexes the style Grams with the old batch stride
        (void)hipGraphExecDestroy(p->gexec); p->gexec = nullptr; p->gwarm = false;
    }
    p->style_batch = style_batch;
    p->have_style = true;
    return ST3D_OK;
}

static int plan_loss_enqueue(st3d_plan *p, const float *current, int n, int batch_denom, float style_weight,
                             float content_weight, float *loss_out, float *grad_current, const uint8_t *need_mask, const float *flat_color, hipStream_t s,
                             Keyed *key = nullptr);

// What the flat and the keyed entry ask of a call alike (`who`: the entry, as its own argument checks name it).  Drops
// *flat_color where the forward runs in full: ST3D_FLAT=0 (A/B runs, read per call), a size without lists, an unaligned image.
static int check_loss_call(const char *who, const st3d_plan *p, const float *current, int n, int batch_denom, const float **flat_color) {
#define LOSS_CALL_ARG(cond)         /* ST3D_CHECK_ARG, under the entry's name */ \
    do {                                                                         \
        if (!(cond)) {                                                           \
            st3d::set_error("%s: invalid argument: %s", who, #cond);             \
            return ST3D_E_INVALID;                                               \
        }                                                                        \
    } while (0)
    if (*flat_color) {
        const char *fl = getenv("ST3D_FLAT");
        if ((fl && fl[0] == '0') || p->d.flat_levels < 1 || ((uintptr_t)current & 15) != 0) *flat_color = nullptr;
    }
    LOSS_CALL_ARG(n > 0 && n <= p->B && batch_denom >= n);
    if (!p->have_content || !p->have_style) {
        st3d::set_error("st3d_plan_loss: content/style targets not set");
        return ST3D_E_STATE;
    }
    LOSS_CALL_ARG(p->style_batch == 1 || p->style_batch == n);
    if (p->guide_n != 0 && p->guide_n != n) {
        st3d::set_error("st3d_plan_loss: the style guidance was set for %d images, this call brings %d", p->guide_n, n);
        return ST3D_E_STATE;
    }
    return ST3D_OK;
#undef LOSS_CALL_ARG
}

extern "C" int st3d_plan_graph(st3d_plan *p, int enable) {
    ST3D_CHECK_ARG(p);
    p->use_graph = enable ? 1 : 0;
    if (!enable && p->gexec) { (void)hipGraphExecDestroy(p->gexec); p->gexec = nullptr; }
    p->gwarm = false;
    return ST3D_OK;
}

extern "C" int st3d_plan_loss(st3d_plan *p, const float *current, int n, int batch_denom, float style_weight,
                              float content_weight, float *loss_out, float *grad_current, st3d_stream_t stream) {
    return st3d_plan_loss_masked(p, current, n, batch_denom, style_weight, content_weight, loss_out, grad_current, nullptr, stream);
}

extern "C" int st3d_plan_loss_masked(st3d_plan *p, const float *current, int n, int batch_denom, float style_weight,
                                     float content_weight, float *loss_out, float *grad_current, const uint8_t *need_mask,
                                     st3d_stream_t stream) {
    return st3d_plan_loss_flat(p, current, n, batch_denom, style_weight, content_weight, loss_out, grad_current, need_mask, nullptr, stream);
}

extern "C" int st3d_plan_loss_flat(st3d_plan *p, const float *current, int n, int batch_denom, float style_weight,
                                   float content_weight, float *loss_out, float *grad_current, const uint8_t *need_mask,
                                   const float *flat_color, st3d_stream_t stream) {
    ST3D_CHECK_ARG(p && current && loss_out);
    p->clean.clear();           // (before anything can fail or replay a graph: an unkeyed call fills whatever it lists)
    p->ls = &p->sets[0];
    ST3D_CHECK_ARG(((uintptr_t)need_mask & 15) == 0);
    if (!grad_current || p->d.need_levels < 1) need_mask = nullptr;      // nothing to thin out: the ordinary call
    ST3D_TRY(check_loss_call(__func__, p, current, n, batch_denom, &flat_color));
    hipStream_t s = st3d::as_stream(stream);
    if (!p->use_graph || p->prof)
        return plan_loss_enqueue(p, current, n, batch_denom, style_weight, content_weight, loss_out, grad_current, need_mask, flat_color, s);

    // ---- graph replay
    const size_t img = (size_t)n * 3 * p->S * p->S;
    const GraphKey key{n, batch_denom, grad_current != nullptr, need_mask != nullptr, flat_color != nullptr, style_weight, content_weight,
                       p->guide_n != 0};
    if (!(p->gexec && key == p->gkey)) {
        if (p->gexec) { (void)hipGraphExecDestroy(p->gexec); p->gexec = nullptr; }
        const bool warm = p->gwarm && key == p->gkey;
        p->gkey = key;
        if (!warm) {            // first call with these parameters: run it plainly (loads every code object, nothing to capture yet)
            p->gwarm = true;
            return plan_loss_enqueue(p, current, n, batch_denom, style_weight, content_weight, loss_out, grad_current, need_mask, flat_color, s);
        }
        hipGraph_t graph = nullptr;
        // captured on a stream of the plan's own: the caller's stream is usually the (uncapturable) default stream
        if (!p->cap_stream) ST3D_HIP(hipStreamCreateWithFlags(&p->cap_stream, hipStreamNonBlocking));
        ST3D_HIP(hipStreamBeginCapture(p->cap_stream, hipStreamCaptureModeThreadLocal));
        const int rc = plan_loss_enqueue(p, p->g_in, n, batch_denom, style_weight, content_weight, p->g_loss,
                                         key.want_grad ? p->g_grad : nullptr, key.masked ? p->g_mask : nullptr,
                                         key.flat ? p->g_color : nullptr, p->cap_stream);
        const hipError_t e = hipStreamEndCapture(p->cap_stream, &graph);
        if (rc != ST3D_OK || e != hipSuccess || !graph) {
            if (graph) (void)hipGraphDestroy(graph);
            if (rc == ST3D_OK) st3d::set_error("st3d_plan_loss: stream capture failed: %s", hipGetErrorString(e));
            return rc != ST3D_OK ? rc : ST3D_E_HIP;
        }
        const hipError_t ei = hipGraphInstantiate(&p->gexec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ei != hipSuccess) { p->gexec = nullptr; st3d::set_error("st3d_plan_loss: hipGraphInstantiate: %s", hipGetErrorString(ei)); return ST3D_E_HIP; }
    }
    ST3D_HIP(hipMemcpyAsync(p->g_in, current, img * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (key.masked) ST3D_HIP(hipMemcpyAsync(p->g_mask, need_mask, (size_t)n * p->S * p->S, hipMemcpyDeviceToDevice, s));
    if (key.flat) ST3D_HIP(hipMemcpyAsync(p->g_color, flat_color, 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    ST3D_HIP(hipGraphLaunch(p->gexec, s));
    ST3D_HIP(hipMemcpyAsync(loss_out, p->g_loss, 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (grad_current) ST3D_HIP(hipMemcpyAsync(grad_current, p->g_grad, img * sizeof(float), hipMemcpyDeviceToDevice, s));
    p->last_n = n;
    return ST3D_OK;
}

// st3d_plan_loss_flat for a caller that knows when the coverage of its views is the one it brought before (a geometry epoch:
// vertices, faces and cameras unchanged, only the texture moves).  Everything that depends on the coverage alone is then
// kept: the need lists and the flat-field lists -- the latter from the coverage, not the pixels -- are built by the first
// call of an epoch, and the fills are launched only when the buffers do not hold this epoch's background already (the
// clean record of st3d_plan).  Results are bitwise those of st3d_plan_loss_flat.
extern "C" int st3d_plan_loss_keyed(st3d_plan *p, const float *current, int n, int batch_denom, float style_weight,
                                    float content_weight, float *loss_out, float *grad_current, const uint8_t *cover,
                                    const float *flat_color, const float *flat_rgb, uint64_t epoch, st3d_stream_t stream) {
    ST3D_CHECK_ARG(p);
    // no epoch, or graph replay (whose captured sequence stays static): the unkeyed call, launch for launch
    if (epoch == 0 || p->use_graph || !cover)
        return st3d_plan_loss_flat(p, current, n, batch_denom, style_weight, content_weight, loss_out, grad_current, cover, flat_color, stream);
    const st3d::CleanRecord held = p->clean;
    p->clean.clear();           // a call refused below leaves it cleared; one that goes through sets it again
    p->ls = &p->sets[0];
    ST3D_CHECK_ARG(current && loss_out && (!flat_color || flat_rgb));
    ST3D_CHECK_ARG(((uintptr_t)cover & 15) == 0);
    const uint8_t *need_mask = (grad_current && p->d.need_levels >= 1) ? cover : nullptr;
    ST3D_TRY(check_loss_call(__func__, p, current, n, batch_denom, &flat_color));
    bool fresh = false;
    const int slot = p->epochs.take(epoch, n, &fresh);
    st3d_plan::ListSet *ls = &p->sets[1 + slot];
    if (fresh) ls->have_need = ls->have_flat = ls->have_kept = ls->have_grp_fwd = ls->have_grp_need = false;
    Keyed key{epoch, cover, flat_rgb, 0, 0};
    p->ls = ls;
    p->clean = held;            // what forward() compares this call with, and clears
    const int rc = plan_loss_enqueue(p, current, n, batch_denom, style_weight, content_weight, loss_out, grad_current, need_mask, flat_color,
                                     st3d::as_stream(stream), &key);
    p->ls = &p->sets[0];
    if (rc != ST3D_OK) {        // whatever the slot holds may be half built, and so may the buffers
        p->epochs.drop(slot);
        p->clean.clear();
        return rc;
    }
    if (key.flat_done > 0) p->clean.set(epoch, n, key.flat_done, flat_rgb, p->vgg->sets, key.kept_done);
    return ST3D_OK;
}

// The backward of the loss step for images [i0, i0 + n) of the last forward: the whole batch, or one group of a split call.
struct BwdArgs {
    int n, i0, batch_denom;
    float content_weight;
    const float *style_coef;            // (host, 5)
    float *grad;                        // the caller's gradient, from image i0 on
    const uint8_t *need_mask;           // likewise (NULL: no lists)
    int need;                           // levels listed
    bool need_gram;
    const st3d_plan::Lists &lists;      // the need lists, numbered from image i0
    float *g0, *g1;                     // the two gradient buffers of this chain and the bytes of each
    size_t gbytes;
};
static int backward_chain(st3d_plan *p, const BwdArgs &b, hipStream_t s) {
    const int n = b.n, need = b.need;
    const bool guided = p->guide_n != 0;
    const int mc = kContentTap;
    const size_t chw = (size_t)p->C[mc] * p->H[mc] * p->W[mc];
    auto act = [&](int m) { return p->at(p->act[m], m, b.i0); };
    auto Dof = [&](int st) { const int m = kStyleTap[st]; return p->D[st] + (size_t)b.i0 * p->C[m] * p->C[m]; };
    const float *content_target = p->content_target + (size_t)b.i0 * chw;
    const float *style_coef = b.style_coef;
    float *grad_current = b.grad;
    const uint8_t *need_mask = b.need_mask;

    // ---- backward: gradient w.r.t. the post-ReLU output of each conv, top down
    float *g = b.g0, *gn = b.g1;
    bool have_g = false, g_is_pooled = false, g_gated = false, content_done = false;
    int pool_of_g = -1;
    const float cc = (float)(2.0 * (double)b.content_weight / ((double)b.batch_denom * (double)chw));       // d content / d conv4_2 = cc * (F - target)
    for (int cs = 12; cs >= 0; --cs) {          // conv slots 12 (module 28) .. 0
        const int m = kConvIdx[cs];
        const int C = p->C[m], H = p->H[m], W = p->W[m];
        int st = -1;
        for (int i = 0; i < 5; ++i)
            if (kStyleTap[i] == m) st = i;
        const Route &r = p->route[cs];
        if (cs == 0 && (st >= 0 || have_g) && p->fused_tap0) {       // relu1_1 and conv1_1 in one pass (tap0.hip)
            Scope sc(p, need >= 1 ? F_CONVX_DGRAD_NEED : F_CONVX_DGRAD, s, m);
            if (guided && st >= 0)
                ST3D_TRY(st3d_conv1_bwd_weighted(have_g ? g : nullptr, act(m), Dof(st), style_coef[st], p->vgg->wd[0], gn,
                                                 b.gbytes, grad_current, n, H, W, p->guide_w0,
                                                 need >= 1 ? b.lists.need_seg : nullptr, need >= 1 ? need_mask : nullptr, s));
            else if (need >= 1)
                ST3D_TRY(st3d_conv1_bwd_masked(have_g ? g : nullptr, act(m), st >= 0 ? Dof(st) : nullptr,
                                               st >= 0 ? style_coef[st] : 0.f, p->vgg->wd[0], gn, b.gbytes,
                                               grad_current, n, H, W, b.lists.need_seg, need_mask, s));
            else
            ST3D_TRY(st3d_conv1_bwd(have_g ? g : nullptr, act(m), st >= 0 ? Dof(st) : nullptr, st >= 0 ? style_coef[st] : 0.f,
                                    p->vgg->wd[0], gn, b.gbytes, grad_current, n, H, W, s));
            break;
        }
        const bool chain = r.gate_taps && !g_is_pooled;
        if (st >= 0 && cs == 2 && need >= 3 && b.need_gram && chain) {        // relu2_1 over the runs conv2_1's input gradient reads
            Scope sc(p, F_GRAM_BWD_NEED, s, m);
            ST3D_TRY(st3d_gram_bwd_gated_segs(Dof(st), act(m), guided ? p->guide_plane(st) : nullptr, n, C, H * W, style_coef[st],
                                              have_g ? 1 : 0, b.lists.need_gram_list, b.lists.need_gram_cnt, g, s));
            g_gated = true;
            have_g = true;
        } else if (st >= 0) {
            Scope sc(p, F_GRAM_BWD, s, m);
            if (guided) {
                ST3D_TRY(st3d_gram_bwd_weighted(Dof(st), act(m), p->guide_plane(st), n, C, H * W, style_coef[st], have_g ? 1 : 0,
                                                chain ? 1 : 0, g, s));
                g_gated = chain;
            } else if (chain) {
                ST3D_TRY(st3d_gram_bwd_gated(Dof(st), act(m), n, C, H * W, style_coef[st], have_g ? 1 : 0, g, s));
                g_gated = true;
            } else {
                ST3D_TRY(st3d_gram_bwd(Dof(st), act(m), n, C, H * W, style_coef[st], have_g ? 1 : 0, g, s));
                g_gated = false;
            }
            have_g = true;
        }
        if (m == kContentTap && !content_done) {
            Scope sc(p, F_ELEM, s);
            if (chain) {
                ST3D_TRY(st3d_axpy_diff_gated(act(m), content_target, (size_t)n * C * H * W, cc, have_g ? 1 : 0, g, s));
                g_gated = true;
            } else {
                ST3D_TRY(st3d_axpy_diff(act(m), content_target, (size_t)n * C * H * W, cc, have_g ? 1 : 0, g, s));
                g_gated = false;
            }
            have_g = true;
        }
        if (!have_g) continue;
        float *dst = (cs == 0) ? grad_current : gn;
        DgradOpts o;
        o.pregated = g_gated;
        // the tensor dst is the gradient of = this conv's forward input (previous post-ReLU output, or the pool's output)
        if (r.gate_dst) o.out_gate = act(pool_slot(m - 1) >= 0 ? m - 1 : m - 2);
        if (o.out_gate && m - 2 == kContentTap) {       // dst is the gradient of the content tap: its own term joins in this launch's store
            o.add_target = content_target;
            o.add_coef = cc;
            content_done = true;
        }
        if (cs >= 1 && cs <= ST3D_NEED_MAX_LISTS && need >= cs + 1) {   // conv1_2 .. conv3_3 over their need lists
            o.tile_list = b.lists.need_list[cs - 1];
            o.n_active = b.lists.need_cnt + (cs - 1);
            o.tile_cols = p->d.need_cols[cs - 1];
        }
        ST3D_TRY(dgrad_step(p, cs, g, g_is_pooled, pool_of_g, dst, n, s, o, b.i0));
        g_gated = o.out_gate != nullptr;
        // dst is the gradient w.r.t. this conv's input: either the previous conv's post-ReLU
        // output or a pool output (then the next dgrad fuses the unpool)
        g_is_pooled = (m > 0) && pool_slot(m - 1) >= 0;
        pool_of_g = g_is_pooled ? pool_slot(m - 1) : -1;
        float *t = g; g = gn; gn = t;
    }
    return ST3D_OK;
}

static int plan_loss_enqueue(st3d_plan *p, const float *current, int n, int batch_denom, float style_weight,
                             float content_weight, float *loss_out, float *grad_current, const uint8_t *need_mask, const float *flat_color, hipStream_t s,
                             Keyed *key) {
    {
        st3d::TraceRange tr("vgg_forward");
        ST3D_TRY(forward(p, current, n, 28, false, s, flat_color, key));
    }
    st3d::TraceRange tr_loss("gram_and_losses");
    const bool guided = p->guide_n != 0;        // (== n: checked by the caller)

    const double bd = (double)batch_denom;
    // content loss: mean over (B,C,H,W) of (F - Ft)^2            (losses.py:31)
    // style loss: sum_l mean over (B,C,C) of (G - S)^2 / (C^2 H^2) (losses.py:34-39)
    // -- the five Grams first, then all six squared-difference sums, their finish and the weighted total in one launch pair
    const int mc = kContentTap;
    const size_t chw = (size_t)p->C[mc] * p->H[mc] * p->W[mc];
    st3d_sqdiff_item items[6];
    items[0] = st3d_sqdiff_item{p->act[mc], p->content_target, nullptr, (size_t)n * chw, (size_t)n * chw,
                                (float)(1.0 / (bd * (double)chw)), 1};
    float style_coef[5];
    {
        Scope sc(p, F_GRAM_FWD, s);
        ST3D_TRY(grams_of_taps(p, n, p->gram, s, guided));
    }
    for (int i = 0; i < 5; ++i) {
        const int m = kStyleTap[i];
        const double C = p->C[m], Hh = p->H[m];
        const size_t cc = (size_t)p->C[m] * p->C[m];
        const double norm = 1.0 / (bd * C * C) / (C * C * Hh * Hh);
        items[1 + i] = st3d_sqdiff_item{p->gram[i], p->style_gram[i], p->D[i], (size_t)n * cc,
                                        p->style_batch == 1 ? cc : (size_t)n * cc, (float)norm, 2};
        style_coef[i] = (float)(4.0 * (double)style_weight * norm);   // d/dF = 2*(dG + dG^T)/2 ... = 4 w norm D F
    }
    {
        Scope sc(p, F_ELEM, s);
        ST3D_TRY(st3d_sqdiff_sum_multi(items, 6, p->partials, loss_out, 1, 1, style_weight, content_weight, s));
    }
    if (!grad_current) return ST3D_OK;
    st3d_trace_pop();                                  // (gram_and_losses ends here; its guard pops "vgg_backward" below)
    st3d_trace_push("vgg_backward");

    // ---- what the consumer of the image gradient needs (need.hip): with a mask, the bottom launches walk these lists
    const int need = need_mask ? p->d.need_levels : 0;
    st3d_plan::ListSet *ls = p->ls;
    if (need > 0 && !(key && ls->have_need)) {          // (a keyed call builds them once per epoch)
        ST3D_TRY(build_need_lists(p, ls->whole, need_mask, n, need, need >= 3 && p->d.need_gram, s));
        if (key) ls->have_need = true;
    }
    BwdArgs b{n, 0, batch_denom, content_weight, style_coef, grad_current, need_mask, need, need >= 3 && p->d.need_gram, ls->whole,
              p->gbuf[0], p->gbuf[1], p->gbuf_floats * sizeof(float)};
    // the split is the clean call's (the forward's condition: this call set flat_done / kept_done and cleared nothing since)
    // The Gram backward's tile height is the one launch parameter written to follow the workgroup count, so B -- but only behind
    // C % 128 == 0, where the 128 x 64 tiling is chosen first: as the launcher stands the choice depends on C and HW alone.  Its
    // tuning knob can bring the count back in (gram.hip reads it per call), so a process that sets it keeps the one-stream call.
    const bool gram_knob = getenv("ST3D_GRAM_BWD_MT") != nullptr;
    if (key && key->clean_call && need_mask && need >= 1 && p->d.need_blocks && !gram_knob && split_ok(p, SPLIT_BWD, n, true)) {
        const int h = n / 2, gneed = std::min(need, p->d.grp_need_levels);
        const bool ggram = gneed >= 3 && p->d.grp_need_gram;
        const size_t img = (size_t)h * p->S * p->S, half = p->gbuf_floats / 2;
        for (int g = 0; g < 2 && !ls->have_grp_need; ++g)
            ST3D_TRY(build_need_lists(p, ls->grp[g], need_mask + g * img, h, gneed, ggram, s));
        ls->have_grp_need = true;
        return run_split(p, 1, s, [&](int g, hipStream_t gs) {
            BwdArgs bg{h, g * h, batch_denom, content_weight, style_coef, grad_current + g * 3 * img, need_mask + g * img, gneed, ggram,
                       ls->grp[g], p->gbuf[0] + g * half, p->gbuf[1] + g * half, half * sizeof(float)};
            return backward_chain(p, bg, gs);
        });
    }
    return backward_chain(p, b, s);
}

// Backward of st3d_plan_forward for external losses on the taps (differentiable get_features, style_transfer.py:61-83):
// grad_modules[m] (host array of kModules device pointers, NULL = no gradient) is d loss / d (output of VGG module m) for
// the n images of the LAST forward, whose activations (post-ReLU outputs, pooled values, argmax) are still in the plan.
// A conv module and the in-place ReLU behind it are the same tensor, so gradients given for either are
// summed.  -> grad_image (n,3,S,S).
extern "C" int st3d_plan_backward(st3d_plan *p, int n, int upto_module, const float *const *grad_modules, float *grad_image,
                                  st3d_stream_t stream) {
    ST3D_CHECK_ARG(p && grad_modules && grad_image);
    ST3D_CHECK_ARG(n > 0 && n <= p->B && n == p->last_n && upto_module >= 0 && upto_module < kModules);
    st3d::TraceRange tr("vgg_backward");
    hipStream_t s = st3d::as_stream(stream);
    float *g = p->gbuf[0], *gn = p->gbuf[1];
    bool have_g = false, g_is_pooled = false;
    int pool_of_g = -1;
    int top = -1;
    for (int cs = 0; cs < 16; ++cs)
        if (kConvIdx[cs] <= upto_module) top = cs;
    for (int m = 0; m < kModules; ++m)
        if (grad_modules[m] && m > upto_module) {
            st3d::set_error("st3d_plan_backward: gradient given for module %d beyond the forward's last module %d", m, upto_module);
            return ST3D_E_INVALID;
        }
    auto blocks = [](size_t cnt) { const size_t b = (cnt + 255) / 256; return (unsigned)(b > 65535 * 16 ? 65535 * 16 : b); };
    for (int cs = top; cs >= 0; --cs) {
        const int m = kConvIdx[cs];
        const int C = p->C[m], H = p->H[m], W = p->W[m];
        const size_t full = (size_t)n * C * H * W;
        const int ps = (m + 2 < kModules && m + 2 <= upto_module) ? pool_slot(m + 2) : -1;
        // (1) a gradient on the pool behind this conv joins the pooled-resolution gradient from above
        if (ps >= 0 && grad_modules[m + 2]) {
            Scope sc(p, F_ELEM, s);
            const size_t pooled = (size_t)n * C * p->H[m + 2] * p->W[m + 2];
            add_kernel<<<blocks(pooled), 256, 0, s>>>(grad_modules[m + 2], pooled, have_g ? 1 : 0, g);
            ST3D_LAUNCH_CHECK();
            have_g = true; g_is_pooled = true; pool_of_g = ps;
        }
        // (2) gradients on the conv's own (post-ReLU) output
        for (int k = 0; k < 2; ++k) {
            const float *tap = (m + k <= upto_module) ? grad_modules[m + k] : nullptr;
            if (!tap) continue;
            Scope sc(p, F_ELEM, s);
            if (have_g && g_is_pooled) {        // bring the pooled gradient to full resolution first, adding the tap on the way
                const size_t pooled = (size_t)n * C * (H / 2) * (W / 2);
                const bool odd = (H & 1) || (W & 1);          // MaxPool2d floors: the last row / column has no window
                if (odd) ST3D_HIP(hipMemsetAsync(gn, 0, full * sizeof(float), s));
                unpool_add_kernel<<<(unsigned)((pooled + 255) / 256), 256, 0, s>>>(g, p->pidx[pool_of_g], odd ? nullptr : tap,
                                                                                (size_t)n * C, H, W, gn);
                ST3D_LAUNCH_CHECK();
                if (odd) { add_kernel<<<blocks(full), 256, 0, s>>>(tap, full, 1, gn); ST3D_LAUNCH_CHECK(); }
                float *t = g; g = gn; gn = t;
                g_is_pooled = false; pool_of_g = -1;
            } else {
                add_kernel<<<blocks(full), 256, 0, s>>>(tap, full, have_g ? 1 : 0, g);
                ST3D_LAUNCH_CHECK();
            }
            have_g = true;
        }
        if (!have_g) continue;
        float *dst = (cs == 0) ? grad_image : gn;
        ST3D_TRY(dgrad_step(p, cs, g, g_is_pooled, pool_of_g, dst, n, s));
        g_is_pooled = (m > 0) && pool_slot(m - 1) >= 0;
        pool_of_g = g_is_pooled ? pool_slot(m - 1) : -1;
        float *t = g; g = gn; gn = t;
    }
    if (!have_g) ST3D_HIP(hipMemsetAsync(grad_image, 0, (size_t)n * 3 * p->S * p->S * sizeof(float), s));
    return ST3D_OK;
}

// how many calls ran their forward / their backward as two groups since the plan was made (either pointer may be NULL)
extern "C" int st3d_plan_split_calls(const st3d_plan *p, int *forward_calls, int *backward_calls) {
    ST3D_CHECK_ARG(p);
    if (forward_calls) *forward_calls = p->split_calls[0];
    if (backward_calls) *backward_calls = p->split_calls[1];
    return ST3D_OK;
}

extern "C" int st3d_plan_profile(st3d_plan *p, int enable) {
    ST3D_CHECK_ARG(p);
    p->prof = enable != 0;
    return ST3D_OK;
}

static int drain_events(st3d_plan *p);

// per-launch records (family * 100 + VGG module index, milliseconds) gathered since the last call; returns how many
extern "C" int st3d_plan_profile_launches(st3d_plan *p, int *tags_out, float *ms_out, int capacity, int *count_out) {
    ST3D_CHECK_ARG(p && count_out && capacity >= 0);
    ST3D_TRY(drain_events(p));
    const int n = (int)p->l_tag.size();
    for (int i = 0; i < n && i < capacity; ++i) {
        if (tags_out) tags_out[i] = p->l_tag[i];
        if (ms_out) ms_out[i] = p->l_ms[i];
    }
    *count_out = n;
    if (capacity >= n) { p->l_tag.clear(); p->l_ms.clear(); }
    return ST3D_OK;
}

extern "C" int st3d_plan_profile_read(st3d_plan *p, float *ms_out, int *launches_out) {
    ST3D_CHECK_ARG(p);
    ST3D_TRY(drain_events(p));
    for (int i = 0; i < ST3D_PROFILE_FAMILIES; ++i) {
        if (ms_out) ms_out[i] = p->fam_ms[i];
        if (launches_out) launches_out[i] = p->fam_n[i];
        p->fam_ms[i] = 0.f;
        p->fam_n[i] = 0;
    }
    return ST3D_OK;
}

static int drain_events(st3d_plan *p) {
    for (auto &e : p->evs) {
        ST3D_HIP(hipEventSynchronize(e.b));
        float ms = 0.f;
        ST3D_HIP(hipEventElapsedTime(&ms, e.a, e.b));
        p->fam_ms[e.fam] += ms;
        p->fam_n[e.fam] += 1;
        p->l_tag.push_back(e.fam * 100 + e.module);
        p->l_ms.push_back(ms);
        p->pool.push_back(e.a);
        p->pool.push_back(e.b);
    }
    p->evs.clear();
    if (p->l_tag.size() > (1u << 20)) { p->l_tag.clear(); p->l_ms.clear(); }      // nobody is reading them
    return ST3D_OK;
}
