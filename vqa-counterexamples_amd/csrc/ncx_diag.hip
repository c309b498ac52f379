// ncx_diag.hip -- the diagnostics ABI: launch timing, in-kernel stamps, the WgMap self-check and the plan query.
#include "ncx_driver.h"
#include "ncx_bf16.h"
#include <stdlib.h>

using namespace ncx;

// ncx_diag_gemm: the description checked against what the engine implements, then turned into the GemmArgs every caller builds.
namespace {
int diag_operand(const ncx_diag_operand& o, XDesc& x) {
    if (o.kind < X_PLAIN || o.kind > X_SOFTMAX || o.rows < 1 || o.cols < 4 || o.ld < o.cols || o.idx_stride < 1) return NCX_E_DIMS;
    if (!o.base || ((o.kind == X_GATHER || o.kind == X_GATHER_MUL) && !o.idx) || (o.kind == X_GATHER_MUL && !o.idx2) ||
        (o.kind == X_SOFTMAX && !o.lse2)) return NCX_E_NULL;
    x = XDesc{};
    x.base = o.base; x.idx = o.idx; x.idx2 = o.idx2; x.mx = o.lse2; x.ld = o.ld; x.kind = o.kind; x.rows = o.rows; x.cols = o.cols;
    x.idx_stride = o.idx_stride;
    return NCX_OK;
}
int diag_gemm_args(const ncx_diag_gemm_args* d, GemmArgs& g, GemmPlan& pl) {
    if (!d) return NCX_E_NULL;
    if (d->form < FORM_NT || d->form > FORM_NN || !cfg_supported(d->form, d->cfg)) return NCX_E_DIMS;
    if ((d->mode != MODE_CHAIN && d->mode != MODE_GROUP) || d->nseg < 1 || d->nseg > NCX_MAX_SEG || d->nseg > NCX_DIAG_MAX_SEG || d->M < 1) return NCX_E_DIMS;
    if (d->act < 0 || d->act > 2 || d->dropout < 0 || d->dropout > 2 || d->rowsplit_g < 0) return NCX_E_DIMS;
    if (d->fold && (d->form != FORM_NT || d->mode != MODE_CHAIN || d->cfg != CFG_64x64)) return NCX_E_DIMS;
    g = GemmArgs{};
    g.mode = d->mode; g.nseg = d->nseg; g.M = d->M;
    const bool a_colk = d->form != FORM_TN, b_colk = d->form == FORM_NT;
    const int np = d->mode == MODE_GROUP ? d->nseg : 1;
    bool any_split = false;
    for (int i = 0; i < d->nseg; ++i) {
        int rc = diag_operand(d->a[i], g.a[i]); if (rc) return rc;
        rc = diag_operand(d->b[i], g.b[i]); if (rc) return rc;
        const int p = d->mode == MODE_GROUP ? i : 0, N = d->n_cols[p], k = d->klen[i];
        if (N < 1 || k < 1) return NCX_E_DIMS;
        // the reduction runs along the columns of a col-is-k operand and along the rows of a row-is-k one; the other extent is M / N
        if ((a_colk ? d->a[i].cols : d->a[i].rows) != k || (a_colk ? d->a[i].rows : d->a[i].cols) != d->M) return NCX_E_DIMS;
        if ((b_colk ? d->b[i].cols : d->b[i].rows) != k || (b_colk ? d->b[i].rows : d->b[i].cols) != N) return NCX_E_DIMS;
        g.klen[i] = k;
    }
    for (int p = 0; p < np; ++p) {
        if (!d->out[p]) return NCX_E_NULL;
        if (d->ldo[p] < d->n_cols[p]) return NCX_E_DIMS;
        g.out[p] = d->out[p]; g.ldo[p] = d->ldo[p]; g.n_cols[p] = d->n_cols[p];
        g.split[p] = d->split[p] > 1 ? d->split[p] : 1;
        any_split |= g.split[p] > 1;
    }
    EpiArgs& e = g.epi;
    e.rowadd = d->rowadd; e.ld_rowadd = d->ld_rowadd; e.rowdiv = d->rowdiv; e.bias = d->bias; e.relu = d->act;
    e.dropout = d->dropout; e.drop_p = d->drop_p; e.drop_scale = d->drop_scale; e.seed_lo = d->seed_lo; e.seed_hi = d->seed_hi; e.layer = d->layer;
    e.keep_mask = d->keep_mask; e.ld_mask = d->ld_mask; e.gate = d->gate; e.ld_gate = d->ld_gate; e.gate_scale = d->gate_scale;
    e.rowsplit_g = d->rowsplit_g; e.out0 = d->out0; e.ldo0 = d->ldo0;
    int n_max = 0;
    for (int p = 0; p < np; ++p) n_max = d->n_cols[p] > n_max ? d->n_cols[p] : n_max;
    if (d->rowadd && (d->rowdiv < 1 || d->ld_rowadd < n_max)) return NCX_E_DIMS;
    if ((d->dropout == 2 && d->ld_mask < n_max) || (d->gate && d->ld_gate < n_max) || (d->rowsplit_g > 0 && d->ldo0 < n_max)) return NCX_E_DIMS;
    if (d->fold && d->ld_fold < (int64_t)d->nseg * n_max) return NCX_E_DIMS;
    if (d->dropout == 2 && !d->keep_mask) return NCX_E_NULL;
    if (d->rowsplit_g > 0 && !d->out0) return NCX_E_NULL;
    if (d->fold) {
        if (!d->fold_mul || !d->fold_bias) return NCX_E_NULL;
        if (d->fold_div < 1) return NCX_E_DIMS;
        e.fold_mul = d->fold_mul; e.fold_bias = d->fold_bias; e.ld_fold = d->ld_fold; e.fold_div = d->fold_div;
    }
    // a split launch's fix-up applies bias and activation only
    if (any_split && (d->rowadd || d->dropout || d->gate || d->rowsplit_g > 0 || d->fold)) return NCX_E_DIMS;
    pl.cfg = d->cfg; pl.split = 1;
    return NCX_OK;
}
}  // namespace

extern "C" {
int ncx_diag_cfg_supported(int32_t form, int32_t cfg) { return cfg_supported(form, cfg) ? 1 : 0; }

size_t ncx_diag_gemm_slab_bytes(const ncx_diag_gemm_args* d) {
    GemmArgs g; GemmPlan pl;
    if (diag_gemm_args(d, g, pl) != NCX_OK) return 0;
    return gemm_slab_bytes(g, pl);
}

int ncx_diag_gemm(ncx_diag_gemm_args* d, void* stream) {
    GemmArgs g; GemmPlan pl;
    int rc = diag_gemm_args(d, g, pl);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!d->fold && gemm_slab_bytes(g, pl) > 0 && !d->slab) return NCX_E_NULL;
    // the FOLD launch does not pass the driver: its no_fast bit is set here
    if (d->fold) { g.pad_ = d->no_fast ? 1 : 0; rc = run_gemm_nt_fold(g, s); }
    else rc = run_gemm_planned(g, d->form, pl, d->slab, d->slab_bytes, nullptr, s, d->no_fast != 0);
    d->grid = g.grid_;
    return rc;
}

int ncx_diag_plan_gemm(int32_t form, int64_t M, int64_t N, int64_t ksteps, int32_t allow_96, int32_t* out2) {
    if (!out2) return NCX_E_NULL;
    if (form < FORM_NT || form > FORM_NN || M < 1 || N < 1 || ksteps < 1) return NCX_E_DIMS;
    const GemmPlan p = plan_gemm(form, M, N, ksteps, allow_96 != 0);
    out2[0] = p.cfg; out2[1] = p.split;
    return NCX_OK;
}

int ncx_profile_begin(uint32_t gemm_mask, int32_t max_launches) {
    if (g_prof.on || gemm_mask == 0 || (gemm_mask >> U_COUNT) != 0 || max_launches < 1 || max_launches > 65536) return NCX_E_DIMS;
    g_prof.ev = (hipEvent_t*)malloc(sizeof(hipEvent_t) * 2 * (size_t)max_launches);
    g_prof.ids = (int*)malloc(sizeof(int) * (size_t)max_launches);
    if (!g_prof.ev || !g_prof.ids) return NCX_E_NULL;
    for (int i = 0; i < 2 * max_launches; ++i) NCX_HIP_TRY(hipEventCreate(&g_prof.ev[i]));
    g_prof.mask = gemm_mask; g_prof.n = 0; g_prof.cap = max_launches; g_prof.on = true;
    return NCX_OK;
}

int ncx_profile_end(float* ms, int32_t* ids, int32_t cap) {
    if (!g_prof.on) return NCX_E_FLAGS;
    int n = 0;
    for (int i = 0; i < g_prof.n; ++i) {
        if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) break;
        float t = 0.f;
        if (hipEventElapsedTime(&t, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) break;
        if (n < cap) { if (ms) ms[n] = t; if (ids) ids[n] = g_prof.ids[i]; }
        ++n;
    }
    for (int i = 0; i < 2 * g_prof.cap; ++i) (void)hipEventDestroy(g_prof.ev[i]);
    free(g_prof.ev); free(g_prof.ids);
    g_prof.ev = nullptr; g_prof.ids = nullptr; g_prof.on = false; g_prof.mask = 0; g_prof.n = 0; g_prof.cap = 0;
    return n < cap ? n : cap;
}

int ncx_profile_stamps(unsigned long long* stamps, int64_t words) {
    if ((stamps == nullptr) != (words == 0) || words < 0) return NCX_E_DIMS;
    int dev = 0;
    NCX_HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16) return NCX_E_DIMS;
    // armed for the CURRENT device only (the buffer lives there); disarm = pointer first, so no reader pairs the old pointer with 0 words
    if (!stamps) { g_stamps[dev].ptr.store(nullptr, std::memory_order_release); g_stamps[dev].words.store(0, std::memory_order_release); }
    else { g_stamps[dev].ptr.store(nullptr, std::memory_order_release); g_stamps[dev].words.store(words, std::memory_order_release);
           g_stamps[dev].ptr.store(stamps, std::memory_order_release); }
    return NCX_OK;
}

int ncx_wgmap_check(int32_t tiles_m, int32_t tiles_n, int32_t S) {
    if (tiles_m < 1 || tiles_n < 1 || S < 1 || (long long)tiles_m * tiles_n * S > (1 << 24)) return NCX_E_DIMS;
    const WgMap w{tiles_m, tiles_n, S};
    const int total = tiles_m * tiles_n * S, count = w.count();
    if (count < total) return 1;
    unsigned char* seen = (unsigned char*)calloc((size_t)total, 1);
    if (!seen) return NCX_E_NULL;
    int bad = 0, nvalid = 0;
    for (int lw = 0; lw < count && !bad; ++lw) {
        int tm = -1, tn = -1, z = -1;
        if (!w.decode(lw, tm, tn, z)) continue;
        ++nvalid;
        if (tm < 0 || tm >= tiles_m || tn < 0 || tn >= tiles_n || z < 0 || z >= S) { bad = 2; break; }
        if (w.encode(tm, tn, z) != lw) { bad = 3; break; }
        unsigned char& f = seen[((size_t)z * tiles_m + tm) * tiles_n + tn];
        if (f) { bad = 4; break; }
        f = 1;
    }
    if (!bad && nvalid != total) bad = 5;
    free(seen);
    return bad;
}

int ncx_bf16_layout(const ncx_dims* d, int32_t* out10) {
    if (check_dims(d) != NCX_OK) return NCX_E_DIMS;
    if (!out10) return NCX_E_NULL;
    const Bf16Cols c = bf16_cols(*d);
    const int32_t v[10] = {c.c_vk, c.c_vm, c.c_misc, c.c_z, c.c_p, c.raw, c.kc, bf16_hp(*d), bf16_up128(d->da), bf16_up128(d->A)};
    for (int i = 0; i < 10; ++i) out10[i] = v[i];
    return NCX_OK;
}

int ncx_plan_query(const ncx_dims* d, int32_t gemm_id, int32_t* out6) {
    if (check_dims(d) != NCX_OK || !out6) return NCX_E_DIMS;
    if (gemm_id == NCX_QUERY_DW1_ROUTE) {      // the routes of linear_1's weight gradient, from the predicates backward_impl launches by
        const bool bf16 = d->flags & NCX_F_BF16;
        const StepRoutes r = routes(*d);
        out6[0] = r.km_form;
        out6[1] = (bf16 ? r.tn8_shared : r.tn8) ? (r.tn8_x6 ? 2 : 1) : 0;
        int grid = 0;
        out6[2] = dw_tn8_pieces(*d, bf16 ? TN8_LIST_SHARED : TN8_LIST_MAIN, &grid);
        out6[3] = grid;
        out6[4] = r.dw1ak_on_tn8(km_defers_to_side_stream(*d, r)) ? 1 : 0;
        out6[5] = TN8_MAX_SEG;
        return NCX_OK;
    }
    if (gemm_id == NCX_QUERY_FUSED_ADAM) {
        const bool on = fused_adam_route(*d, routes(*d)) && ((size_t)d->A * d->da) % 4 == 0;
        for (int i = 0; i < 6; ++i) out6[i] = 0;
        out6[0] = on ? 1 : 0;
        out6[1] = on ? main_adam_passengers() : 0;
        return NCX_OK;
    }
    if (gemm_id == NCX_QUERY_BF16_ROUTE) {     // the kernel selections of the bf16 variant, from the function its launchers launch by
        for (int i = 0; i < 6; ++i) out6[i] = 0;
        if (!(d->flags & NCX_F_BF16)) { out6[0] = -1; return NCX_OK; }
        const Bf16Route b = bf16_route(*d);
        out6[0] = b.nt_form; out6[1] = b.tn8; out6[2] = b.S; out6[3] = b.chunk; out6[4] = b.nz; out6[5] = b.vec;
        return NCX_OK;
    }
    if (gemm_id == NCX_QUERY_GTSH_PAIR) {      // Gt and Sh as one launch: the route forward_impl takes and the joint plan it launches by
        const StepRoutes r = routes(*d);
        SideStream* ss = side_stream();
        out6[0] = r.gtsh_pair(*d, ss && ss->mode != 3) ? 1 : 0;
        out6[1] = r.pair_s_gt; out6[2] = r.pair_s_sh;
        out6[3] = r.pair_w_gt; out6[4] = r.pair_w_sh;
        out6[5] = 3 * num_cus();
        return NCX_OK;
    }
    if (gemm_id == NCX_QUERY_FWD_ROUTE) {      // the forward's Linear layers, from the functions forward_impl and main_forward launch by
        const StepRoutes r = routes(*d);
        GemmUse u[U_COUNT];
        list_uses(*d, r, u);
        const long long M = (long long)d->B * d->K;
        const bool bf16 = d->flags & NCX_F_BF16;
        for (int i = 0; i < 6; ++i) out6[i] = 0;
        if (bf16) out6[0] = 3;
        else if (main_fwd_dims_ok(*d)) {
            const FwdRoute f = forward_route(*d, r);
            const int sp = main_split(M, d->H, r.cand_ksteps);
            out6[0] = f.vfold ? 2 : 1;
            out6[1] = f.vfold ? main_fold_rows_eff(M, d->H, d->K) : main_chain_form(M, d->H, r.cand_ksteps, sp, false, true);
            out6[2] = sp;
            out6[3] = f.dist_in_main ? 1 : 0;
        } else { out6[1] = u[U_MAIN].plan.cfg; out6[2] = u[U_MAIN].plan.split; }
        if (d->L < 2) { out6[4] = -1; return NCX_OK; }
        if (hidden_fwd_dims_ok(*d) && !bf16) { out6[4] = 1; out6[5] = main_split(M, d->H, ksteps(d->H)); }
        else out6[5] = u[U_FWD_L].plan.split;
        return NCX_OK;
    }
    if (gemm_id < 0 || gemm_id >= U_COUNT) return NCX_E_DIMS;
    GemmUse u[U_COUNT];
    list_uses(*d, routes(*d), u);
    out6[0] = u[gemm_id].form; out6[1] = (int32_t)u[gemm_id].M; out6[2] = (int32_t)u[gemm_id].N;
    out6[3] = (int32_t)u[gemm_id].ksteps; out6[4] = u[gemm_id].plan.cfg; out6[5] = u[gemm_id].plan.split;
    // linear_1 / hidden-layer forward: the fused kernel of ncx_main.h (tile codes 5: 48x128, 6: 48x64 with the per-triplet fold)
    const bool fast = (gemm_id == U_MAIN && main_fwd_dims_ok(*d)) || (gemm_id == U_FWD_L && hidden_fwd_dims_ok(*d) && !(d->flags & NCX_F_BF16));
    if (fast) {
        const long long M = (long long)d->B * d->K, T = u[gemm_id].ksteps;
        const int sp = main_split(M, d->H, T);
        const bool vfold = gemm_id == U_MAIN && (d->flags & NCX_F_V_MULT) && (d->K == 24 || (d->K == 48 && main_fold_rows(M, d->H) >= 96)) && d->dv % 32 == 0 && d->dv >= 64 && sp == 1;
        const long long tiles96 = ((M + 95) / 96) * ((d->H + 127) / 128);
        out6[4] = vfold ? (main_fold_rows(M, d->H) == 192 ? 8 : (main_fold_rows(M, d->H) == 96 || d->K == 48) ? 7 : 6) : (sp == 1 && tiles96 * 10 >= (long long)num_cus() * 9) ? CFG_96x128 : 5;
        out6[5] = sp;
    }
    return NCX_OK;
}
}  // extern "C"
