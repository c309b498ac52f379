// ncx_plan.hip -- the planner of one step (host only): dims check, split-K plans, the step's routes, the GEMM uses and the
// workspace layout.  forward / backward and the workspace size all read the same StepRoutes, GemmUse list and WsLayout.
#include "ncx_plan.h"
#include "ncx_bf16.h"
#include <stdio.h>

namespace ncx {
int check_dims(const ncx_dims* d) {
    if (!d) return NCX_E_NULL;
    if (d->B < 1 || d->K < 1 || d->K > 64 || d->dv < 1 || d->dq < 1 || d->dz < 1 || d->da < 1 || d->A < 1 ||
        d->H < 1 || d->L < 1 || d->L > 3 || d->n_img < 1)
        return NCX_E_DIMS;
    if ((long long)d->B * d->K > (1ll << 30) / 4 || d->B > NCX_SCATTER_MAX_B) return NCX_E_DIMS;
    if (d->dv < 4 || d->dq < 4 || d->dz < 4 || d->da < 4 || d->A < 4 || d->H < 4 || d->K < 3) return NCX_E_DIMS;   // 16-byte windows
    if (d->drop_p < 0.f || d->drop_p >= 1.f) return NCX_E_DIMS;
    if (d->flags & ~(NCX_F_ALL | NCX_F_BF16 | NCX_F_REUSE_GT | NCX_F_FUSED_TAIL | NCX_F_X6)) return NCX_E_FLAGS;
    if ((d->flags & NCX_F_BF16) && (d->flags & NCX_F_ALL) != NCX_F_ALL) return NCX_E_FLAGS;    // bf16 variant: no lesions
    return NCX_OK;
}

// Padded weight copies (ncx_main.h reads every weight row up to the next multiple of 32 columns).  Slot i of the wpad region:
//   0 v_other  1 v_mult  2 dist | rank  3 z_other  4 a_other (a_emb lesion only)  5 linear_2  6 linear_3
// width 0: the slice is used in place (already a multiple of 32 wide, or the segment does not exist).
int wpad_cols(const ncx_dims& d, int i) {
    const int c[WPAD_N] = {d.dv, (d.flags & NCX_F_V_MULT) ? d.dv : 0, d.K + 1, d.dz, (d.flags & NCX_F_A_EMB) ? 0 : d.da, d.L >= 2 ? d.H : 0, d.L >= 3 ? d.H : 0};
    return c[i];
}
int wpad_width(const ncx_dims& d, int i) {
    const int c = wpad_cols(d, i);
    if (d.flags & NCX_F_BF16) return 0;
    return (c == 0 || c % 32 == 0) ? 0 : pad_to(c, 32);
}

// Split planning.  A problem whose whole tiles cannot fill the chip is split along K into S aligned chunks and
// run as W = tiles*S equal workgroups through the stream-K path (W = tiles*S makes the unit ranges coincide with
// the chunks, so workgroups on the same chunk of different tiles share operand rows in L2; unaligned ranges lost
// that sharing and ran 1.3x slower).  Equal workgroups execute in rounds of `slots` = CUs x resident
// workgroups per CU, so S is chosen to fill whole rounds (1648 workgroups on 512 slots = 3.2 rounds cost 4).
int num_cus() {
    static int n = 0;
    if (!n) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
        else { (void)hipGetLastError(); n = 256; }
    }
    return n;
}

// Measured (DW1C on 512 slots, 412 tiles x 384 k-steps): S = 4/5/6/7/9/12/16/24/32 -> 0.541/0.538/0.521/0.513/
// 0.486/0.486/0.486/0.508/0.525 ms: aim for >= 6 rounds of workgroups but keep >= 24 k-steps in each.
static int choose_split(long long tiles, long long ksteps, long long slots) {
    if (tiles >= slots) return 1;                  // at least one full round of workgroups already (dE at H=1024: 217 us unsplit, 230 us x2)
    long long sp = cdiv(6 * slots, tiles);
    const long long smax = ksteps / 24 > 1 ? ksteps / 24 : 1;
    if (sp > smax) sp = smax;
    if (tiles * sp < slots) {                      // cannot even fill one round: trade pipeline depth for parallelism
        const long long smax2 = ksteps / 8 > 1 ? ksteps / 8 : 1;
        sp = cdiv(slots, tiles);
        if (sp > smax2) sp = smax2;
    }
    return (int)(sp < 1 ? 1 : sp);
}

// tiles_small: output tiles with 64x64 blocks; ksteps: 32-deep reduction steps per tile.
static GemmPlan plan_from_tiles(int form, long long tiles_big, long long tiles_small, long long ksteps, bool big_ok) {
    GemmPlan p; p.split = 1;
    // 128x128 tiles run one workgroup per CU: only when they fill whole rounds of CUs reasonably (dE at H=1024: 304 tiles =
    // 1.19 rounds took 362 us, the 64x64 plan 217 us)
    const long long cus = num_cus();
    const double eff_big = (double)tiles_big / (double)(cdiv(tiles_big, cus) * cus);
    if (big_ok && tiles_big >= 192 && ksteps >= 64 && eff_big >= 0.75) { p.cfg = CFG_128x128; return p; }
    // Measured on MI355X (DW1C, 412 small tiles x 384 k-steps): every TN tile shape (64x64, 128x64, 128x128) ends
    // at 0.45-0.51 ms; the 64x64 tile fits 3 workgroups per CU and is used for all split problems.
    p.cfg = CFG_64x64;
    const int occ = form == FORM_NT ? occupancy_nt(p.cfg) : form == FORM_TN ? occupancy_tn(p.cfg) : occupancy_nn(p.cfg);
    p.split = choose_split(tiles_small, ksteps, (long long)occ * num_cus());
    return p;
}

GemmPlan plan_gemm(int form, long long M, long long N, long long ksteps, bool allow_96) {
    // Epilogue GEMMs (forward layers) never split; both big NT tiles run one workgroup per CU, so pick the one
    // whose tile count fills whole rounds of CUs better (H=512: 384 tiles of 128x128 = 1.5 rounds, 512 of 96x128 = 2).
    // Short reductions (<= 32 k-steps, e.g. the 360-wide MUTAN / classifier products): the per-workgroup prologue and
    // epilogue of the big tiles dominate; measured at M=12288, N=2000, K=360: 645 / 335 / 245 us for 128x128 / 96x128 / 64x64.
    if (form == FORM_NT && allow_96 && ksteps <= 32 && M * N >= 64 * 64 * 512) {
        GemmPlan p; p.cfg = CFG_64x64; p.split = 1; return p;
    }
    if (form == FORM_NT && allow_96 && M >= 96 && N >= 128) {
        const double cus = (double)num_cus();
        const double t128 = (double)(cdiv(M, 128) * cdiv(N, 128)), t96 = (double)(cdiv(M, 96) * cdiv(N, 128));
        const double waste128 = (double)(cdiv(M, 128) * 128 * cdiv(N, 128) * 128) / (double)(M * N);
        const double waste96 = (double)(cdiv(M, 96) * 96 * cdiv(N, 128) * 128) / (double)(M * N);
        const double e128 = (t128 / cus) / (double)cdiv((long long)t128, (long long)cus) / waste128;
        const double e96 = (t96 / cus) / (double)cdiv((long long)t96, (long long)cus) / waste96;
        if (t96 >= 0.75 * cus || t128 >= 0.75 * cus) {
            GemmPlan p; p.split = 1; p.cfg = e96 > e128 * 1.02 ? CFG_96x128 : CFG_128x128; return p;
        }
    }
    const bool big_ok = M >= 96 && N >= 96;
    return plan_from_tiles(form, cdiv(M, 128) * cdiv(N, 128), cdiv(M, 64) * cdiv(N, 64), ksteps, big_ok);
}

StepRoutes routes(const ncx_dims& d) {
    StepRoutes r{};
    const bool bf16 = d.flags & NCX_F_BF16, aemb = d.flags & NCX_F_A_EMB, km_ok = dw_km_supported(d);
    r.km = km_ok && !bf16;
    r.km_form = bf16 ? KM_FORM_NONE : km_ok ? dw_km_form(d) : KM_FORM_GROUPED;
    r.tn8 = dw_tn8_supported(d);
    r.tn8_shared = dw_tn8_shared_ok(d);
    r.tn8_x6 = dw_tn8_x6(d);
    // NT form of the answer-embedding gradient: the fp32 path with the a_emb segment on (ncx_train_tail and backward_impl fill
    // the dGt^T | dGgt^T block in that form, ncx_ws_region names it)
    r.emb_nt = aemb && !bf16 && !hook_env("NCX_NO_EMB_NT");
    // ... over rows permuted so that the answers of the batch come first: the row tiles behind them skip the dGgt^T segment (all zeros there)
    r.de_skip = r.emb_nt && d.A <= NCX_PERM_MAX_A && !hook_env("NCX_NO_DE_SKIP");
    r.cand_ksteps = ksteps(d.dv) * ((d.flags & NCX_F_V_MULT) ? 2 : 1) + ksteps(d.K + 1) + ksteps(d.dz) + ksteps(aemb ? d.A : d.da);
    // Gt and Sh as one launch: fp32 path with the a_emb segment on, every reduction extent a multiple of 4 (16-byte operand windows), operand
    // extents below 4 GiB, and a joint plan that splits at least one of the two (else today's launches already fill the chip or have nothing to cut)
    r.pair_s_gt = r.pair_s_sh = 1; r.pair_w_gt = r.pair_w_sh = 0;
    r.pair_ok = false;
    if (aemb && !bf16 && d.dv % 4 == 0 && d.dq % 4 == 0 && d.dz % 4 == 0 && d.da % 4 == 0 && main_fwd_extents_ok(d) &&
        (long long)d.B * d.dq * 4 < (1ll << 32) - 65536 && !hook_env("NCX_NO_GTSH_PAIR")) {
        const PairPlan p = plan_gtsh_pair(d, r);
        r.pair_s_gt = p.s_gt; r.pair_s_sh = p.s_sh; r.pair_w_gt = p.w_gt; r.pair_w_sh = p.w_sh;
        r.pair_ok = p.w_gt > 0 && (p.s_gt > 1 || p.s_sh > 1);
    }
    return r;
}

// The splits of the pair are those the generic engine's plans give the two problems on launches of their own (list_uses: U_GT, U_SH; both cut a
// chain of T steps into S chunks [T z / S, T (z + 1) / S) and sum a 32-deep step in one order), and the fix-up adds the partial tiles z
// ascending like split_fixup2_kernel: Gt and Sh are then the two-launch path's bit for bit, and a training run keeps its trajectory.  What
// the joint plan chooses is how many WORKGROUPS share a tile's chunks: w_gt | S_gt, w_sh | S_sh, a workgroup running S / w consecutive chunks.
// The kernel deals its (row tile, workgroup) units round-robin over the 8 XCDs and keeps a unit's column tiles on one XCD, so the round that
// must hold is the round of EVERY XCD: ceil(units / 8) x column tiles of both problems together within 3 x CUs / 8 slots -- with Gt's 32
// column tiles per unit a plan that fits the chip as a whole (3 and 10 workgroups per tile at configs[1]: 704 of 768 slots) still puts 104
// workgroups on the 96 slots of four XCDs, and the launch waits for their second round (measured: 58.5 us against 65.9 for the two launches
// it replaces).  Among the (w_gt, w_sh) that fit every XCD's round: the pair whose longest workgroup is shortest (the launch is as
// long as its slowest workgroup and what shares its CU), then the one that leaves the fullest XCD the fewest tile-steps.  configs[1]: S = 4 /
// 16 as on the generic engine, 4 / 8 workgroups per tile, 768 in all, 64 + 32 on every XCD (two of Gt and one of Sh per CU).
// w_gt == 0: no plan (another tile form, or even one workgroup per tile overfills an XCD).
PairPlan plan_gtsh_pair(const ncx_dims& d, const StepRoutes& r) {
    PairPlan p{};
    const long long tm_gt = cdiv(d.H, 64), tn_gt = cdiv(d.A, 64), tm_sh = cdiv(d.B, 64), tn_sh = cdiv(d.H, 64);
    p.tiles_gt = tm_gt * tn_gt; p.t_gt = ksteps(d.da);
    p.tiles_sh = tm_sh * tn_sh; p.t_sh = ksteps(d.dv) + ksteps(d.dq) + ksteps(d.dz) + ksteps(d.da);
    p.slots = 3ll * num_cus();
    p.s_gt = p.s_sh = 1; p.w_gt = p.w_sh = 0;
    GemmUse u[U_COUNT];
    list_uses(d, r, u);
    if (u[U_GT].plan.cfg != CFG_64x64 || u[U_SH].plan.cfg != CFG_64x64) return p;
    p.s_gt = u[U_GT].plan.split > 1 ? u[U_GT].plan.split : 1;
    p.s_sh = u[U_SH].plan.split > 1 ? u[U_SH].plan.split : 1;
    if (p.s_gt > p.t_gt || p.s_sh > p.t_sh) return p;
    if (const char* e = hook_env("NCX_PAIR_WPT")) {      // experiment hook (NCX_EXPERIMENT=1): "w_gt,w_sh", the workgroups per tile (divisors of the splits, else no plan)
        int wg = 0, ws = 0;
        if (sscanf(e, "%d,%d", &wg, &ws) == 2 && wg >= 1 && ws >= 1 && p.s_gt % wg == 0 && p.s_sh % ws == 0) { p.w_gt = wg; p.w_sh = ws; }
        return p;
    }
    const long long xcd_slots = p.slots / 8;
    long long best_work = -1, best_long = 0;
    for (long long wg = 1; wg <= p.s_gt; ++wg)
        for (long long ws = 1; ws <= p.s_sh; ++ws) {
            if (p.s_gt % wg || p.s_sh % ws) continue;
            const long long n_gt = cdiv(tm_gt * wg, 8) * tn_gt, n_sh = cdiv(tm_sh * ws, 8) * tn_sh;      // workgroups of the fullest XCD
            if (n_gt + n_sh > xcd_slots) continue;
            const long long cg = cdiv(p.t_gt, wg), cs = cdiv(p.t_sh, ws), lng = cg > cs ? cg : cs;
            const long long work = n_gt * cg + n_sh * cs;                                                // ... and its tile-steps
            if (best_work < 0 || lng < best_long || (lng == best_long && work < best_work)) { best_work = work; best_long = lng; p.w_gt = (int)wg; p.w_sh = (int)ws; }
        }
    return p;
}

int pair_wpad_width(const ncx_dims& d, const StepRoutes& r, int i) {
    const int c[PAIR_WPAD_N] = {d.dv, d.dq, d.dz, d.da, d.da};
    return (!r.pair_ok || c[i] % 32 == 0) ? 0 : pad_to(c[i], 32);
}

// Split of one candidate-column problem of the grouped dW1 launch.  The big problems (2048 / 2000 columns) fill whole
// rounds of workgroup slots; the narrow ones (dist + rank: 25 columns, z_other: 360) are dispatched after them and would
// keep a few CUs busy for a full-length tail: they get twice as many, shorter k-chunks (still >= 8 k-steps each).
int dw1c_seg_split(long long cols, int S, long long ksteps) {
    long long narrow = 512;
    if (const char* e = hook_env("NCX_SMALL_COLS")) narrow = atoll(e);
    if (S <= 1 || cols > narrow) return S;
    int mult = 2;                     // measured at C2: x1 0.445-0.450 ms, x2 0.427, x3 0.438, x4 0.443
    if (const char* e = hook_env("NCX_SMALL_MULT")) mult = atoi(e) > 0 ? atoi(e) : 1;
    long long sp = (long long)S * mult;
    const long long smax = ksteps / 8 > 1 ? ksteps / 8 : 1;
    if (sp > smax) sp = smax;
    return (int)(sp < S ? S : sp);
}

void list_uses(const ncx_dims& d, const StepRoutes& r, GemmUse* u) {
    const long long M = (long long)d.B * d.K, H = d.H;
    const bool aemb = d.flags & NCX_F_A_EMB;
    const long long cand_cols = (long long)d.dv * ((d.flags & NCX_F_V_MULT) ? 2 : 1) + d.K + 1 + d.dz + (aemb ? d.A : d.da);
    const long long sh_k = ksteps(d.dv) + ksteps(d.dq) + ksteps(d.dz) + ksteps(d.da);
    const long long sh_cols = (long long)d.dv + d.dq + d.dz + d.da;
    u[U_GT]    = {FORM_NT, H, d.A, ksteps(d.da), false};
    u[U_SH]    = {FORM_NT, d.B, H, sh_k, false};
    u[U_MAIN]  = {FORM_NT, M, H, r.cand_ksteps, true};
    u[U_FWD_L] = {FORM_NT, M, H, ksteps(H), true};
    u[U_DW1C]  = {FORM_TN, H, cand_cols, ksteps(M), false};
    u[U_DW1S]  = {FORM_TN, H, sh_cols, ksteps(d.B), false};
    u[U_DE]    = {FORM_TN, d.A, d.da, 2 * ksteps(H), false};
    u[U_DW1AK] = {FORM_NN, H, d.da, ksteps(d.A), false};
    u[U_DAGT]  = {FORM_NN, 1, 1, 1, false};                 // (folded into U_DE)
    u[U_DWL]   = {FORM_TN, H, H, ksteps(M), false};
    u[U_DXL]   = {FORM_NN, M, H, ksteps(H), false};
    const bool hooks = experiment_hooks_on();
    // grouped launches (DW1C + DW1S): tiles are counted per column segment.  The v_other / v_mult columns leave for ncx_dwkm.hip (km),
    // every other column block + dGt for ncx_dwtn.hip (tn8; the bf16 variant: its fp32 shared segments take the TN kernel too)
    const bool km = r.km, tn8 = r.tn8, tn8s = r.tn8_shared;
    const long long segs_c[5] = {km ? 0 : d.dv, (!km && (d.flags & NCX_F_V_MULT)) ? d.dv : 0, tn8 ? 0 : d.K + 1, tn8 ? 0 : d.dz, tn8 ? 0 : (aemb ? d.A : d.da)};
    const long long segs_s[5] = {tn8s ? 0 : d.dv, tn8s ? 0 : d.dq, tn8s ? 0 : d.dz, tn8s ? 0 : d.da, 0};
    for (int i = 0; i < U_COUNT; ++i) {
        const bool grouped = i == U_DW1C || i == U_DW1S;
        auto grouped_tiles = [&](int bm, int bn) {
            const long long* sg = i == U_DW1C ? segs_c : segs_s;
            long long t = 0;
            for (int q = 0; q < 5; ++q) t += cdiv(H, bm) * cdiv(sg[q], bn);
            return t;
        };
        if (grouped && grouped_tiles(64, 64) == 0) {      // nothing left for the grouped launch
            u[i].plan.cfg = CFG_128x64; u[i].plan.split = 1;
        } else if (grouped) {
            u[i].plan = plan_from_tiles(FORM_TN, grouped_tiles(128, 128), grouped_tiles(64, 64), u[i].ksteps, false);
            // Measured on MI355X (C2, H=256: 206 tiles of 128x64 x 384 k-steps): 128x64 with 6-8 k-chunks 0.448 ms vs
            // 0.476 ms for 64x64 x 8; three rounds of the 2-per-CU slots.
            if (i == U_DW1C && H >= 128 && u[i].plan.split > 1) {
                u[i].plan.cfg = CFG_128x64;
                const long long slots = (long long)occupancy_tn(CFG_128x64) * num_cus();
                long long sp = cdiv(3 * slots, grouped_tiles(128, 64));
                const long long smax = u[i].ksteps / 24 > 1 ? u[i].ksteps / 24 : 1;
                if (sp > 8) sp = 8;          // one k-chunk per XCD at most (measured with the fused v-column kernel: x8 0.346, x12 0.354, x16 0.363 ms)
                u[i].plan.split = (int)(sp > smax ? smax : sp < 1 ? 1 : sp);
            }
        } else {
            u[i].plan = plan_gemm(u[i].form, u[i].M, u[i].N, u[i].ksteps, u[i].allow96);
        }
        if (i == U_MAIN || i == U_FWD_L || i == U_DXL) u[i].plan.split = 1;       // epilogue GEMMs never split
        if (hooks) {   // experiment hooks (NCX_EXPERIMENT=1): NCX_SPLIT_<id>=S forces S aligned k-chunks, NCX_CFG_<id> the tile config
            char name[32];
            snprintf(name, sizeof name, "NCX_CFG_%d", i);
            const char* c = getenv(name);
            if (c && cfg_supported(u[i].form, atoi(c))) u[i].plan.cfg = atoi(c);      // a tile the form does not instantiate: ignored
            snprintf(name, sizeof name, "NCX_SPLIT_%d", i);
            const char* e = getenv(name);
            if (e && i != U_MAIN && i != U_FWD_L && i != U_DXL) u[i].plan.split = atoi(e) > 1 ? atoi(e) : 1;
        }
        int bm, bn; cfg_tile(u[i].plan.cfg, bm, bn);
        long long tiles = cdiv(u[i].M, bm) * cdiv(u[i].N, bn);
        if (grouped) tiles = grouped_tiles(bm, bn);
        u[i].tiles = tiles;
        // slab slots = workgroup ids (the chunk-per-XCD layout of WgMap pads some problems)
        const int S = u[i].plan.split > 1 ? u[i].plan.split : 1;
        long long wgs = 0;
        if (grouped) {
            const long long* sg = i == U_DW1C ? segs_c : segs_s;
            for (int q = 0; q < 5; ++q)
                if (sg[q] > 0) wgs += WgMap{(int)cdiv(H, bm), (int)cdiv(sg[q], bn), i == U_DW1C ? dw1c_seg_split(sg[q], S, u[i].ksteps) : S}.count();
        } else {
            wgs = WgMap{(int)cdiv(u[i].M, bm), (int)cdiv(u[i].N, bn), S}.count();
        }
        u[i].wgs = wgs;
        u[i].slab_elems = S > 1 ? wgs * bm * bn : 0;
    }
    // DW1S rides in DW1C's launch (same tile config): its workgroups' slab slots follow DW1C's
    u[U_DW1S].plan.cfg = u[U_DW1C].plan.cfg;
    {
        int bm, bn; cfg_tile(u[U_DW1C].plan.cfg, bm, bn);
        const int S = u[U_DW1S].plan.split > 1 ? u[U_DW1S].plan.split : 1;
        u[U_DW1S].tiles = 0; u[U_DW1S].wgs = 0;
        for (int q = 0; q < 4; ++q) {
            if (segs_s[q] == 0) continue;
            u[U_DW1S].tiles += cdiv(H, bm) * cdiv(segs_s[q], bn);
            u[U_DW1S].wgs += WgMap{(int)cdiv(H, bm), (int)cdiv(segs_s[q], bn), S}.count();
        }
        u[U_DW1C].slab_elems = (u[U_DW1C].wgs + u[U_DW1S].wgs) * bm * bn;
        u[U_DW1S].slab_elems = 0;
    }
}

WsLayout ws_layout(const ncx_dims& d) { return ws_layout(d, routes(d)); }
WsLayout ws_layout(const ncx_dims& d, const StepRoutes& r) {
    WsLayout w{};
    const size_t M = (size_t)d.B * d.K, H = d.H;
    WsCarver cv;
    w.idx_k = cv.take(M * 4); w.idx_o = cv.take(M * 4); w.idx_ob = cv.take((size_t)d.B * 4);
    w.mx = cv.take(M * 4); w.inv = cv.take(M * 4);
    w.ldm = pad_to(d.K + 1, 4);
    w.ldgt = (d.flags & NCX_F_BF16) ? d.A : pad_to(d.A, 32);
    w.misc = cv.take(M * w.ldm * 4);
    w.gt = cv.take(H * w.ldgt * 4);
    w.sh = cv.take((size_t)d.B * H * 4);
    for (int l = 0; l < 3; ++l) w.h[l] = l < d.L ? cv.take(M * H * 4) : 0;
    w.dpre[0] = cv.take(M * H * 4);
    w.dpre[1] = d.L >= 2 ? cv.take(M * H * 4) : 0;
    w.dsh = cv.take((size_t)d.B * H * 4);
    w.dgt = cv.take(2 * H * d.A * 4);                      // dGt[H][A], then (contiguous: one all-reduce bucket under DP)
    w.dagt = w.dgt + H * d.A * 4;                       // dGgt[H][A] = one-hot(aid)^T dSh, transposed
    w.dgtT = cv.take((size_t)2 * d.A * pad_to(d.H, 4) * 4);
    w.w1aT = cv.take((size_t)2 * d.da * pad_to(d.H, 32) * 4);
    w.dgtT2 = cv.take(r.tn8 ? (size_t)pad_to(d.A, 32) * pad_to(d.H, 4) * 4 : 0);
    w.de_perm = cv.take(r.emb_nt ? ((size_t)d.A + 1) * 4 : 0);
    w.partial = cv.take((size_t)NCX_PRELUDE_WAVES * H * 4 * 2 + (size_t)NCX_PRELUDE_WAVES * 4 + 256);     // (>= NCX_COLSUM_CHUNKS rows)
    GemmUse u[U_COUNT];
    list_uses(d, r, u);
    long long slab = 0;
    for (int i = 0; i < U_COUNT; ++i) slab = u[i].slab_elems > slab ? u[i].slab_elems : slab;
    w.slab_bytes = (size_t)slab * 4;
    if (dw_tn8_slab_bytes(d) > w.slab_bytes) w.slab_bytes = dw_tn8_slab_bytes(d);      // ncx_dwtn.hip: its partial tiles live here too
    w.slab = cv.take(w.slab_bytes);
    {   // side-stream GEMMs (Gt, Sh forward; dW1ak, dE backward) get their own slab
        long long s2 = u[U_GT].slab_elems;
        if (u[U_SH].slab_elems > s2) s2 = u[U_SH].slab_elems;
        if (u[U_DW1AK].slab_elems > s2) s2 = u[U_DW1AK].slab_elems;
        if (u[U_DE].slab_elems > s2) s2 = u[U_DE].slab_elems;
        // ... which also holds the partial tiles of the Gt + Sh pair launch: [S_gt][H][A], then [S_sh][B][H]
        const long long pair = r.pair_ok ? (long long)r.pair_s_gt * d.H * d.A + (long long)r.pair_s_sh * d.B * d.H : 0;
        if (pair > s2) s2 = pair;
        w.slab2_bytes = (size_t)s2 * 4;
        w.slab2 = cv.take(w.slab2_bytes);
    }
    w.km_slab = cv.take(dw_km_slab_bytes(d));
    {   // split-K slabs of the fused forward kernel: linear_1 / hidden layers at small batches
        auto need = [&](long long m, long long n, long long t) { const int sp = main_split(m, n, t); return sp > 1 ? (size_t)sp * m * n * 4 : (size_t)0; };
        size_t b = need((long long)M, (long long)H, r.cand_ksteps);
        if (d.L >= 2) b = b > need((long long)M, (long long)H, ksteps(H)) ? b : need((long long)M, (long long)H, ksteps(H));
        w.mslab_bytes = b;
        w.mslab = cv.take(b);
    }
    {   // padded weight copies for the fused forward kernel: [H][pad32(width)] each, in the order pack_wpad fills them
        size_t e = 0;
        for (int i = 0; i < WPAD_N; ++i) e += (size_t)H * wpad_width(d, i);
        w.wpad = cv.take(e * 4);
    }
    if (d.flags & NCX_F_BF16) {                          // packed bf16 operands of the two dominant GEMMs (ncx_bf16.h)
        w.xc = cv.take(bf16_xc_bytes(d)); w.wc = cv.take(bf16_wc_bytes(d));
        w.dpre_bf = cv.take(bf16_dpre_bytes(d)); w.bf_slab = cv.take(bf16_slab_bytes(d));
        w.bf_emb = cv.take(bf16_emb_bytes(d));
    }
    {   // padded weight copies of the Gt + Sh pair launch (last: every other region keeps its place)
        size_t e = 0;
        for (int i = 0; i < PAIR_WPAD_N; ++i) e += (size_t)(i == 4 ? d.A : d.H) * pair_wpad_width(d, r, i);
        w.pwpad = cv.take(e * 4);
    }
    w.total = cv.off;
    return w;
}
}  // namespace ncx
