// Mode N host side, the workspaces: what a problem's solves and builds keep on the device and in pinned memory (NormalWs: every loop's
// part and the general loop's; FusedWs: the single-camera loop's), each ONE planned block from its layout (ccal_normal.hpp), made on
// first use and given back to the context's cache with the problem; the column table; and the tests' two hooks: the poison, which
// every allocation of doubles passes through, and the switch of the one-shot calls' slice guards (ccal_internal.hpp).  The loops that
// use them: ccal_solver.hip.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "ccal_fused.hpp"
#include "ccal_devopt.hpp"

using namespace ccal;
namespace ccal {

hipError_t test_poison_f64(ccal_ctx* ctx, void* p, size_t bytes, bool host, hipStream_t s) {
#ifdef CCAL_TEST_HOOKS
    // read on every call (not cached in a static): tests switch it per case in-process
    const char* e = std::getenv("CCAL_TEST_POISON_ALLOC");
    if (!e || e[0] != '1' || !p || !bytes) return hipSuccess;
    if (host) { std::memset(p, 0xFF, bytes); return hipSuccess; }
    return hipMemsetAsync(p, 0xFF, bytes, s ? s : ctx->stream);
#else
    (void)ctx; (void)p; (void)bytes; (void)host; (void)s;
    return hipSuccess;
#endif
}

bool test_guard_slices() {
#ifdef CCAL_TEST_HOOKS
    const char* e = std::getenv("CCAL_TEST_GUARD_SLICES");       // read on every call, as above
    return e && e[0] == '1';
#else
    return false;
#endif
}

void normal_ws_destroy(ccal_problem* p) {
    NormalWs* w = p->nws;
    if (!w) return;
    // early-exit groups of the last solve (or of a solve that ended in an error: every such exit sets tail_pending) may
    // still be queued: they publish into the pinned status words freed below.  The whole device is drained rather than
    // the stream: the stream may be the caller's own (ccal_ctx_create with a stream) and already destroyed when a
    // binding's garbage collector gets here.
    if (w->tail_pending || (w->fws && w->fws->tail_pending)) {
        (void)hipSetDevice(p->ctx->device);
        (void)hipDeviceSynchronize();
    }
    // (the blocks go back to the context's cache - ccal_internal.hpp - for its next problem; ccal_problem_destroy has drained the stream)
    ccal_ctx* ctx = p->ctx;
    if (w->side) { (void)hipStreamSynchronize(w->side); ctx_stream_put(ctx, w->side); }
    ctx_release(ctx, w->d_base, false); ctx_release(ctx, w->d_block, false); ctx_release(ctx, w->h_block, true);
    if (FusedWs* f = w->fws) {
        if (f->side) { (void)hipStreamSynchronize(f->side); ctx_stream_put(ctx, f->side); }      // (the result's download ran there)
        ctx_release(ctx, f->d_block, false);          // every device buffer of the workspace is a slice of it
        ctx_release(ctx, f->h_block, true);           // h_status | h_result | h_stage
        ctx_release(ctx, f->fcbuf, false);            // (NULL but in -DCCAL_STAMPS builds)
        delete f;
    }
    delete w;
    p->nws = nullptr;
}

int drain_pending_groups(ccal_problem* p) {
    NormalWs* w = p->nws;
    bool any = w && (w->tail_pending || (w->fws && w->fws->tail_pending));
    if (!any) return CCAL_OK;
    ccal_ctx* ctx = p->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const int rc = drain_tail(ctx, ctx->stream, any); rc != CCAL_OK) return rc;
    w->tail_pending = false;
    if (w->fws) w->fws->tail_pending = false;
    return CCAL_OK;
}

int fused_ws_ensure(ccal_problem* p) {
    NormalWs* w = p->nws;
    if (w->fws) return CCAL_OK;
    ccal_ctx* ctx = p->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    FusedWs* f = new FusedWs();
    w->fws = f;
    f->PRAW = praw_size(p->K);
#ifdef CCAL_LEGACY_KERNELS
    { const char* e = dev_env("CCAL_FUSE_ELIM"); f->fuse_elim = !(e && e[0] == '0'); }      // second library: the separate elimination launch (k_schur1m)
#endif
    f->RB1 = fused_red_size(p->K);
    f->n_pw = fused_partial_rows(p->n_obs);
    // ONE device allocation and ONE pinned allocation, sliced (a calibration session creates a problem and solves it once or
    // twice: fifteen device and pinned allocations and five memsets were 0.46 ms of the first solve's 0.58 at 600 frames)
    const FusedLayout l((size_t)p->n_slots, (size_t)p->n_obs, (size_t)w->PF, (size_t)f->PRAW, (size_t)f->RB1, (size_t)f->n_pw);
    HIP_TRY(ctx, ctx_block_alloc(ctx, l.dev, &f->d_block, false));
    HIP_TRY(ctx, ctx_block_alloc(ctx, l.host, &f->h_block, true));
    const Bound d{ f->d_block }, h{ f->h_block };
    for (int i = 0; i < 2; ++i) { f->pf[i] = d.at(l.pf[i]); f->praw[i] = d.at(l.praw[i]); }
    f->partial = d.at(l.partial); f->red = d.at(l.red); f->red_stride = l.red_stride; f->done_cnt = d.at(l.done_cnt);
    f->mc_f = d.at(l.mc_f); f->cost_f = d.at(l.cost_f); f->d_state = d.at(l.state); f->d_stage = d.at(l.d_stage);
    f->h_status = h.at(l.h_status); f->h_result = h.at(l.h_result); f->h_stage = h.at(l.h_stage);
    // per-frame scratch of diagnostic builds (-DCCAL_STAMPS: in-kernel timestamps, tools/stamps_*.py); the product allocates nothing
#ifdef CCAL_STAMPS
    HIP_TRY(ctx, ctx_doubles(ctx, &f->fcbuf, std::max<size_t>((size_t)std::max(p->n_obs, 1) * 40, 32768)));
#endif
    HIP_TRY(ctx, ctx_stream_get(ctx, &f->side));
    return CCAL_OK;
}

// The part every loop needs: sizes, the column table and the camera step.  The single-camera loop (FusedWs) needs nothing else of
// NormalWs; the general loop's buffers - per-frame record sets, slot tables, partial sums, a second status block and stream - are
// made when a general-loop entry first asks (normal_ws_ensure_general): one device block, one pinned block, one upload.
int normal_ws_ensure(ccal_problem* p) {
    if (p->nws) return CCAL_OK;
    ccal_ctx* ctx = p->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    NormalWs* w = new NormalWs();
    p->nws = w;
    w->K = p->K; w->RB = red_size(p->K); w->PF = pf_size(p->K);
    const NormalBaseLayout l;
    HIP_TRY(ctx, ctx_block_alloc(ctx, l.plan, &w->d_base, false));
    w->dc = Bound{ w->d_base }.at(l.dc); w->cols = Bound{ w->d_base }.at(l.cols);
    return CCAL_OK;
}
int normal_ws_ensure_general(ccal_problem* p) {
    int rc0 = normal_ws_ensure(p);
    if (rc0 != CCAL_OK) return rc0;
    NormalWs* w = p->nws;
    if (w->general_ready) return CCAL_OK;
    ccal_ctx* ctx = p->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // persistent wavefronts of k_schur: 4 per SIMD (measured at 10 000 slots x 2 cameras: 2048 -> 165.7, 4096 -> 158.5, 8192 -> 173 us per build)
    int n_pw = std::min(std::max(p->n_slots, 1), std::max(4, dev_env_int("CCAL_SCHUR_WAVES", 4096)));
    n_pw = (n_pw + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK * WAVES_PER_BLOCK;
    // 64 .. 127 columns (five and more cameras): the (K + 1)^2 accumulators of a wavefront take up to 131 KB of LDS - one
    // wavefront per workgroup and CU, 512 of them (each writes its own row of partial sums: 512 x RB doubles)
    // (also below 64 columns when four wavefronts' images do not fit the CU's 160 KB: K + 1 = 62 .. 64 with OPENCV5-sized records)
    {
        int stg = 0;
        for (int c = 0; c < p->n_cams; ++c) stg = std::max(stg, gen_e_off(p->cams[c].Peff) + 144);       // as launch_schur
        const int K1 = p->K + 1;
        const size_t ws4 = sizeof(double) * WAVES_PER_BLOCK * (size_t)((((w->RB + 12 * K1 + 36 + 1) & ~1)) + stg);
        if (p->K >= 64 || ws4 + 6 * 1024 > 160 * 1024) { w->schur_wpb = 1; n_pw = std::min(std::max(p->n_slots, 1), 512); }
    }
    w->n_pw = n_pw;
    std::vector<int64_t> goff(p->n_obs);
    std::vector<int32_t> caminfo(p->n_cams * 4);
    int64_t gl = 0;
    // Register Gram kernels + record format for every camera (k_gram1v / k_gram2, GEN; k_schur expands the records).
    // CCAL_GENERAL_GRAM=mfma: the matrix-core kernel k_gram (ccal_legacy_normal.hip) with its 16 x 16 / 32-stride tiles
    // (19-column other-camera blocks), kept as the independent second implementation the tests compare against.
#ifdef CCAL_LEGACY_KERNELS
    { const char* e = dev_env("CCAL_GENERAL_GRAM"); w->register_gram = !(e && e[0] == 'm') || w->schur_wpb == 1; }      // the matrix-core pair: four-wavefront elimination only
#else
    w->register_gram = true;               // (the matrix-core pair lives in libccal_hip_legacy.so only)
#endif
    // two cameras with equal blocks: k_schurq from 1 000 slots (round 4, with its eight-lanes-per-slot form up to 8 192 slots; whole
    // build against the generic k_schur<true>: 1 000 slots 27.5 against 28.2 us, 3 000: 37.6 / 42.6, 6 000: 56.1 / 63.8, 10 000: 71.7
    // with k_schur at 81); below that the generic kernel's many short wavefronts win.  CCAL_SCHURQ=1 / 0 forces it / the generic
    // k_schur<true>, which every other rig takes
    {
        int pe[CCAL_MAX_CAMS], ct[CCAL_MAX_CAMS], ce[CCAL_MAX_CAMS];
        for (int c = 0; c < p->n_cams; ++c) { pe[c] = p->cams[c].Peff; ct[c] = p->cams[c].col_theta; ce[c] = p->cams[c].col_extr; }
        const char* e = dev_env("CCAL_SCHURQ");
        w->schurq = w->register_gram && schurq_fits(p->n_cams, pe, ct, ce) && (e ? e[0] != '0' : p->n_slots >= 1000);
    }
    w->schurq_slots = schurq_slots_per_wave(p->n_slots);
    { const int v = dev_env_int("CCAL_SCHURQ_SLOTS", 0); if (v == 8 || v == 16) w->schurq_slots = v; }
    w->n_rows = w->schurq ? schurq_rows(p->n_slots, w->schurq_slots) : n_pw / w->schur_wpb;
    // cameras of one model (and the problem's one focal mode): their blocks go through ONE launch (CCAL_MERGE_GRAM=0: one per camera)
    {
        bool same = p->n_cams > 1;
        for (int c = 1; c < p->n_cams; ++c) same = same && p->cams[c].model == p->cams[0].model && p->cams[c].Peff == p->cams[0].Peff;
        const char* e = dev_env("CCAL_MERGE_GRAM");
        w->merged_gram = w->register_gram && same && !(e && e[0] == '0');
    }
    std::vector<int> ncp_of(p->n_cams);
    for (int c = 0; c < p->n_cams; ++c) {
        ncp_of[c] = (p->cams[c].D + 1) <= 16 ? 16 : 32;
        caminfo[c * 4 + 0] = p->cams[c].Peff; caminfo[c * 4 + 1] = p->cams[c].col_theta;
        caminfo[c * 4 + 2] = p->cams[c].col_extr; caminfo[c * 4 + 3] = w->register_gram ? 0 : ncp_of[c];
    }
    if (w->schurq) {
        // k_schurq: a slot's two records side by side at (2 slot + camera) x record size - the kernel computes the addresses and
        // requests the records with its first instructions instead of after a look-up; a missing record is a hole that stays
        // zero (the buffers are cleared below and nothing ever writes there)
        const int64_t rs = gen_rec_size(p->cams[0].Peff);
        for (int o = 0; o < p->n_obs; ++o) goff[o] = (2 * (int64_t)p->h_obs_slot[o] + p->h_obs_cam[o]) * rs;
        gl = 2 * (int64_t)std::max(p->n_slots, 1) * rs;
    } else {
        for (int o = 0; o < p->n_obs; ++o) {
            goff[o] = gl;
            const int c = p->h_obs_cam[o];
            gl += w->register_gram ? (int64_t)gen_rec_size(p->cams[c].Peff) : (int64_t)ncp_of[c] * ncp_of[c];
        }
    }
    w->g_len = gl;
    std::vector<int32_t> slot_off(p->n_slots + 1, 0), slot_obs(p->n_obs);
    for (int o = 0; o < p->n_obs; ++o) slot_off[p->h_obs_slot[o] + 1]++;
    for (int s = 0; s < p->n_slots; ++s) slot_off[s + 1] += slot_off[s];
    { std::vector<int32_t> cur(slot_off.begin(), slot_off.end() - 1);
      for (int o = 0; o < p->n_obs; ++o) slot_obs[cur[p->h_obs_slot[o]]++] = o; }
    std::vector<int64_t> slot_desc(p->n_obs);
    for (int i = 0; i < p->n_obs; ++i) slot_desc[i] = goff[slot_obs[i]] * 8 + p->h_obs_cam[slot_obs[i]];
    std::vector<int8_t> owner(p->n_obs, 0);
    w->all_slots_observed = true;
    for (int sl = 0; sl < p->n_slots; ++sl) {
        if (slot_off[sl + 1] > slot_off[sl]) owner[slot_obs[slot_off[sl]]] = 1;
        else w->all_slots_observed = false;
    }
    std::vector<int32_t> all, sorted[1 + CCAL_MAX_CAMS];
    if (w->merged_gram) for (int c = 0; c < p->n_cams; ++c) all.insert(all.end(), p->cams[c].obs.begin(), p->cams[c].obs.end());
    if (w->register_gram) {
        // ragged frames: every Gram launch's list sorted by corner count, with the bins of the launch (the single-camera loop's plan,
        // ccal_kernels_gram2.hip: gram2_bin_plan - uniform frames and short lists get none)
        auto plan_list = [&](const std::vector<int32_t>& list, int slot, int model) {
            if (list.size() < 2000) return;
            std::vector<int64_t> off(list.size() + 1, 0);
            for (size_t i = 0; i < list.size(); ++i) off[i + 1] = off[i] + (p->h_obs_off[list[i] + 1] - p->h_obs_off[list[i]]);
            std::vector<int32_t> order;
            const GramBins gb = gram2_bin_plan(off.data(), (int)list.size(), model == kUCM || model == kEUCM, &order, true);
            if (gb.n_bins <= 0) return;
            sorted[slot].resize(list.size());
            for (size_t i = 0; i < list.size(); ++i) sorted[slot][i] = list[(size_t)order[i]];
            w->gen_bins[slot] = gb;
        };
        if (w->merged_gram) plan_list(all, 0, p->cams[0].model);
        else for (int c = 0; c < p->n_cams; ++c) plan_list(p->cams[c].obs, 1 + c, p->cams[c].model);
    }
    std::vector<int64_t> slot_rec;
    if (w->schurq) {
        slot_rec.assign((size_t)std::max(p->n_slots, 1) * 2, -1);
        for (int o = 0; o < p->n_obs; ++o) slot_rec[(size_t)p->h_obs_slot[o] * 2 + p->h_obs_cam[o]] = goff[o];
    }
    // ONE device block and ONE pinned block (GeneralLayout, ccal_normal.hpp); the index tables go up as one image with one copy.  The
    // block's clear is ordered on the context's stream (ctx_block_alloc): the kernels rely on what is never written staying zero - holes in the
    // record buffers (tile (1,0) of two-tile blocks, k_schurq's missing records), the upper-triangle rows of `partial` (k_schurq writes the rest)
    size_t n_sorted[1 + CCAL_MAX_CAMS];
    for (int i = 0; i <= CCAL_MAX_CAMS; ++i) n_sorted[i] = sorted[i].size();
    const GeneralLayout l(p->n_cams, (size_t)p->n_obs, (size_t)p->n_slots, (size_t)w->RB, (size_t)w->PF, (size_t)gl, (size_t)std::max(n_pw, w->n_rows),
                          w->merged_gram, w->schurq, n_sorted);
    HIP_TRY(ctx, ctx_block_alloc(ctx, l.dev, &w->d_block, false));
    HIP_TRY(ctx, ctx_block_alloc(ctx, l.host, &w->h_block, true));
    const Bound d{ w->d_block }, h{ w->h_block };
    for (int i = 0; i < 2; ++i) { w->G[i] = d.at(l.G[i]); w->cost_o[i] = d.at(l.cost_o[i]); }
    w->partial = d.at(l.partial); w->mc_slot = d.at(l.mc_slot); w->scal = d.at(l.scal); w->flags = d.at(l.flags);
    w->red = d.at(l.red); w->pf = d.at(l.pf); w->d_gstate = d.at(l.gstate);
    w->h_gstatus = h.at(l.h_gstatus); w->h_gstate = h.at(l.h_gstate); w->h_pinned = h.at(l.h_pinned);
    HIP_TRY(ctx, ctx_stream_get(ctx, &w->side));
    std::vector<char> image(l.dev.total - l.goff.off);          // (read by an asynchronous copy: alive until normal_upload_cols has synchronised)
    auto tab = [&](auto*& ptr, auto slice, const auto& v) {       // a table's address (an optional one that is absent: NULL) and its part of the image
        ptr = d.at(slice);
        if (!v.empty()) std::memcpy(image.data() + (slice.off - l.goff.off), v.data(), v.size() * sizeof(v[0]));
    };
    tab(w->d_goff, l.goff, goff); tab(w->d_slot_off, l.slot_off, slot_off); tab(w->d_slot_obs, l.slot_obs, slot_obs); tab(w->d_obs_cam, l.obs_cam, p->h_obs_cam);
    tab(w->d_caminfo, l.caminfo, caminfo); tab(w->d_slot_desc, l.slot_desc, slot_desc); tab(w->d_obs_owner, l.obs_owner, owner);
    tab(w->d_all_obs, l.all_obs, all); tab(w->d_slot_rec, l.slot_rec, slot_rec);
    for (int i = 0; i <= CCAL_MAX_CAMS; ++i) tab(w->d_gen_sorted[i], l.sorted[i], sorted[i]);
    HIP_TRY(ctx, hipMemcpyAsync(d.at(l.goff), image.data(), image.size(), hipMemcpyHostToDevice, ctx->stream));
    w->general_ready = true;
    return normal_upload_cols(p);
}

void build_cols(const ccal_problem* p, ColInfo* cols) {
    std::memset(cols, 0, CCAL_KMAX * sizeof(ColInfo));
    for (int c = 0; c < p->n_cams; ++c) {
        const CamLayout& cl = p->cams[c];
        for (int i = 0; i < cl.Peff; ++i) {
            ColInfo& ci = cols[cl.col_theta + i];
            // column i of the camera's block is the kernels' canonical parameter `full`; an OPENCV5 coefficient lives at
            // position 4 + ocv5_order[.] of the CALLER's vector: that is where its bounds / fixed flag were set (eff index
            // space of the caller) and where the step goes
            int full = p->one_focal ? (i == 0 ? 0 : i + 1) : i;          // eff -> full index (fy re-inserted)
            if (cl.model == kOCV5 && full >= 4) full = 4 + p->ctx->conv.ocv5_order[full - 4];
            const int q = c * CCAL_PMAX + (full - (p->one_focal && full > 0 ? 1 : 0));
            ci.lo = p->lo[q]; ci.hi = p->hi[q]; ci.has_bound = p->has_bound[q]; ci.fixed = p->fixed[q];
            ci.is_extr = 0;
            ci.dst = c * CCAL_PMAX + full;
            ci.dst2 = (p->one_focal && i == 0) ? c * CCAL_PMAX + 1 : -1;
        }
        if (c > 0) for (int i = 0; i < 6; ++i) {
            ColInfo& ci = cols[cl.col_extr + i];
            ci.is_extr = 1; ci.dst = c * 6 + i; ci.dst2 = -1;
        }
    }
}

// reduced-system column (the kernels' canonical parameter order) -> the same parameter's column in the CALLER's order
// (differs only for OPENCV5 cameras under a non-default ccal_model_conventions.ocv5_order)
void caller_columns(const ccal_problem* p, int* ext) {
    for (int k = 0; k < p->K; ++k) ext[k] = k;
    for (int c = 0; c < p->n_cams; ++c) {
        const CamLayout& cl = p->cams[c];
        if (cl.model != kOCV5) continue;
        const int shift = p->one_focal ? 1 : 0;
        for (int d = 0; d < 5; ++d) ext[cl.col_theta + 4 - shift + d] = cl.col_theta + 4 - shift + p->ctx->conv.ocv5_order[d];
    }
}

int normal_upload_cols(ccal_problem* p) {
    NormalWs* w = p->nws;
    ccal_ctx* ctx = p->ctx;
    std::vector<ColInfo> cols(CCAL_KMAX);
    build_cols(p, cols.data());
    HIP_TRY(ctx, hipMemcpyAsync(w->cols, cols.data(), CCAL_KMAX * sizeof(ColInfo), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CCAL_OK;
}

}  // namespace ccal
