// pz_verify.cpp -- the device batch verifier behind include/pz.h (pz_vk_create, pz_verify_batch): the host side.  Per proof it replays
// the transcript (host/transcript.hpp, the prover's own) and derives the handful of scalars that need an inversion -- one batch inversion
// over the whole batch; everything per member of a proof runs in pz_verify.hip's kernels, the MSM is K1 and the check pz_pairing_check_dev.
// paillier_halo2_amd/verifier.py::verify_batch states the same verdicts in Python integers.
//
// Every proof's commitments are held to the wire decoder's rule for a point first (one launch: the identity, or canonical coordinates on
// the curve); a proof that fails it, states a non-canonical evaluation or misses the identity at x is refused without touching the rest.
// Happy path: one fold with random weights into K1's two columns over [fixed | sigma | g0 | every proof's commitments], ONE MSM, ONE
// 2-pair check.  Otherwise (a failed fold, a failed identity, or the caller asks for each proof's A and B) per-proof checks without a
// B x (all bases) matrix: one B-column MSM over the key's bases and g0, one 2-column MSM per proof over its own commitments (a sub-range
// of the same device array, loaded as a bases set of its own), the two parts added, then B 2-pair checks in one launch.  Device memory
// is O(B (F + m) + the proofs' commitments and evaluations).
#include <errno.h>
#include <sys/random.h>

#include <mutex>
#include <new>
#include <vector>

#include "pz_internal.h"
#include "../host/key_digest.hpp"
#include "../host/transcript.hpp"

using pzh::Fr;

struct pz_vk {
    pz_ctx* ctx = nullptr;
    uint32_t k = 0, bf = 0;
    pz_vshape s{};
    uint32_t set_pts[PZ_VSETS_MAX][4] = {};   // indices into the six rotation points
    uint64_t g2[32] = {};                     // g2 | s_g2: the G2 side of every check
    void* d_vkb = nullptr;                    // fixed | sigma | g0, affine
    void* d_delta = nullptr;                  // delta^c, c < m
    void* d_members = nullptr;                // (evaluation offset, destination) per member of the query sets
    pz_bases* t_vk = nullptr;                 // K1 table of d_vkb (the per-proof checks' vk MSM)
    size_t n_public = 0;                      // values of the instance column (s.n_inst = 1), else 0
    std::vector<uint64_t> commitments;        // fixed | sigma as the caller gave them: what the key's digest is taken over
    std::mutex digest_mu;                     // the digest is computed on the first request (pz_vk_digest, or a bound verification)
    bool have_digest = false, bound = false;  // bound: every proof's replay starts from digest || seed (pz_vk_bind)
    uint8_t digest[pzh::KEY_DIGEST_BYTES] = {};
};

namespace {

struct Fail {
    int rc;
};
void ck(int rc) {
    if (rc != PZ_OK) throw Fail{rc};
}
template <class F> int guarded(F&& f) {
    try {
        f();
        return PZ_OK;
    } catch (const Fail& e) {
        return e.rc;
    } catch (const std::bad_alloc&) {
        return PZ_ERR_OOM;
    } catch (...) {
        return PZ_ERR_INTERNAL;
    }
}
// device block of the context, released on every path
struct Dev {
    pz_ctx* ctx;
    void* d = nullptr;
    explicit Dev(pz_ctx* c) : ctx(c) {}
    ~Dev() {
        if (d) pz_dev_free(ctx, d);
    }
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    void alloc(size_t bytes) { ck(pz_dev_alloc(ctx, bytes ? bytes : 32, &d)); }
    template <class T = uint64_t> T* p() const { return (T*)d; }
};
struct BasesGuard {
    pz_ctx* ctx;
    pz_bases* b = nullptr;
    ~BasesGuard() {
        if (b) pz_bases_free(ctx, b);
    }
};

Fr sub(const Fr& a, const Fr& b) { return pzh::add(a, pzh::neg(b)); }
bool is_zero(const Fr& a) { return !(a.v[0] | a.v[1] | a.v[2] | a.v[3]); }
bool canonical(const uint64_t* v) { return !pzh::ge_mod(v); }

// Montgomery's trick over the whole batch: a[i] <- 1 / a[i]; zeros stay zero
void batch_invert(std::vector<Fr>& a) {
    std::vector<Fr> pre(a.size());
    Fr acc = pzh::FR_ONE;
    for (size_t i = 0; i < a.size(); ++i) {
        pre[i] = acc;
        if (!is_zero(a[i])) acc = pzh::mul(acc, a[i]);
    }
    Fr inv = pzh::inv(acc);
    for (size_t i = a.size(); i-- > 0;) {
        if (is_zero(a[i])) continue;
        const Fr t = pzh::mul(inv, pre[i]);
        inv = pzh::mul(inv, a[i]);
        a[i] = t;
    }
}

bool os_random(void* buf, size_t n) {
    uint8_t* p = (uint8_t*)buf;
    size_t got = 0;
    while (got < n) {
        const ssize_t r = getrandom(p + got, n - got, 0);
        if (r < 0) {
            if (errno == EINTR) continue;
            break;
        }
        got += (size_t)r;
    }
    if (got == n) return true;
    FILE* f = fopen("/dev/urandom", "rb");
    if (!f) return false;
    const bool ok = fread(p + got, 1, n - got, f) == n - got;
    fclose(f);
    return ok;
}

// the layout of a proof and of the query sets (prover.query_layout's order)
void make_shape(size_t A, size_t Lk, size_t n_instance, pz_vk& vk, std::vector<uint32_t>& mem) {
    pz_vshape& s = vk.s;
    const uint32_t F = (uint32_t)A + 2, m = (uint32_t)(A + Lk + 1 + n_instance), S = (m + 1) / 2;
    s.n_inst = (uint32_t)n_instance;
    s.A = (uint32_t)A;
    s.Lk = (uint32_t)Lk;
    s.F = F;
    s.m = m;
    s.S = S;
    s.n_own = s.A + 4 * s.Lk + S + 6;
    s.n_vkb = F + m + 1;
    s.e_adv = 0;
    s.e_lka = 4 * s.A;
    s.e_fix = s.e_lka + s.Lk + 1;
    s.e_sig = s.e_fix + F;
    s.e_pz = s.e_sig + m;
    s.e_lz = s.e_pz + 3 * S;
    s.e_ap = s.e_lz + 2 * s.Lk;
    s.e_sp = s.e_ap + 2 * s.Lk;
    s.e_rnd = s.e_sp + s.Lk;
    s.e_h = s.e_rnd + 1;
    s.n_ev = s.e_h + 1;
    // commitment indices: advice | lookup advice | A' | S' | perm products | lookup products | random | h_0..h_2 | W1 | W2
    const uint32_t c_lka = s.A, c_ap = c_lka + s.Lk, c_sp = c_ap + s.Lk, c_pz = c_sp + s.Lk, c_lz = c_pz + S, c_rnd = c_lz + s.Lk,
                   c_h = c_rnd + 1;
    auto put = [&](uint32_t eoff, uint32_t kind, uint32_t slot) {
        mem.push_back(eoff);
        mem.push_back(kind << 30 | slot);
    };
    uint32_t ns = 0;
    auto open_set = [&](std::initializer_list<uint32_t> pts) {
        s.set_start[ns] = (uint32_t)(mem.size() / 2);
        s.set_npts[ns] = (uint32_t)pts.size();
        uint32_t q = 0;
        for (uint32_t t : pts) vk.set_pts[ns][q++] = t;
    };
    auto close_set = [&]() {
        s.set_count[ns] = (uint32_t)(mem.size() / 2) - s.set_start[ns];
        ++ns;
    };
    open_set({0});
    for (uint32_t i = 0; i < s.Lk; ++i) put(s.e_lka + i, PZ_VM_OWN, c_lka + i);
    for (uint32_t i = 0; i < F; ++i) put(s.e_fix + i, PZ_VM_VK, i);
    for (uint32_t i = 0; i < m; ++i) put(s.e_sig + i, PZ_VM_VK, F + i);
    for (uint32_t i = 0; i < s.Lk; ++i) put(s.e_sp + i, PZ_VM_OWN, c_sp + i);
    put(0, PZ_VM_H, c_h);
    put(s.e_rnd, PZ_VM_OWN, c_rnd);
    close_set();
    open_set({0, 1, 2, 3});
    for (uint32_t i = 0; i < s.A; ++i) put(s.e_adv + 4 * i, PZ_VM_OWN, i);
    close_set();
    if (S > 1) {
        open_set({0, 1, 4});
        for (uint32_t i = 0; i + 1 < S; ++i) put(s.e_pz + 3 * i, PZ_VM_OWN, c_pz + i);
        close_set();
    }
    open_set({0, 1});
    put(s.e_pz + 3 * (S - 1), PZ_VM_OWN, c_pz + S - 1);
    for (uint32_t i = 0; i < s.Lk; ++i) put(s.e_lz + 2 * i, PZ_VM_OWN, c_lz + i);
    close_set();
    open_set({0, 5});
    for (uint32_t i = 0; i < s.Lk; ++i) put(s.e_ap + 2 * i, PZ_VM_OWN, c_ap + i);
    close_set();
    s.n_sets = ns;
}

// the key's digest, computed once per key object
const uint8_t* vk_digest(pz_vk* vk) {
    std::lock_guard<std::mutex> g(vk->digest_mu);
    if (!vk->have_digest) {
        const pz_vshape& s = vk->s;
        pzh::key_digest(vk->k, vk->bf, s.A, s.Lk, s.n_inst, vk->n_public, vk->commitments.data(), vk->commitments.data() + 8ull * s.F, vk->digest);
        vk->have_digest = true;
    }
    return vk->digest;
}

// what the host derives for one proof once the transcript is replayed
struct Replay {
    Fr beta, gamma, y, x, sy, sv, su;
    bool canon = true;
    size_t inv0 = 0;   // its first entry in the batch's inversion list
};

// stated_h: the proofs carry h(x) as their last evaluation and must state the value the expression implies (pz_verify_batch); proofs that
// came in as wire bytes do not send it (their slot is zero) and the comparison does not apply
void verify(pz_vk* vk, const uint64_t* proofs, size_t B, const uint8_t* seeds, const size_t* seed_off, int32_t* verdicts,
            uint64_t* h_evals, uint64_t* ab_affine, int* all_ok, bool stated_h = true, const uint64_t* instances = nullptr) {
    pz_ctx* ctx = vk->ctx;
    const pz_vshape& s = vk->s;
    const size_t cw = 8ull * s.n_own, ew = 4ull * s.n_ev, pw = cw + ew;
    const uint64_t n = 1ull << vk->k;
    const uint64_t u_row = n - (vk->bf + 1);
    const Fr w = pzh::omega(vk->k), one = pzh::FR_ONE, nf = pzh::from_u64(n);
    const Fr w_u = pzh::pow_u64(w, u_row), w_m1 = pzh::pow_u64(w, n - 1);
    const uint32_t c_ap = s.A + s.Lk, c_pz = s.A + 3 * s.Lk, c_h = c_pz + s.S + s.Lk + 1;
    const size_t NP = vk->n_public;

    // 1. transcripts, then everything that needs an inversion, inverted at once
    const uint8_t* bind = vk->bound ? vk_digest(vk) : nullptr;   // a bound key: digest || seed where the seed alone stood
    std::vector<Replay> rp(B);
    std::vector<Fr> inv;
    std::vector<std::vector<Fr>> pts(B);
    for (size_t i = 0; i < B; ++i) {
        const uint64_t* c = proofs + i * pw;
        const uint64_t* e = c + cw;
        static const uint8_t none = 0;
        pzp::Transcript tr(bind, seeds ? (const void*)(seeds + seed_off[i]) : (const void*)&none, seed_off[i + 1] - seed_off[i]);
        Replay& r = rp[i];
        if (NP) {   // the statement: absorbed after the seed, before the first commitment; a value >= r is no statement (verdict 0)
            std::vector<uint64_t> im(4 * NP, 0);
            for (size_t j = 0; j < NP && r.canon; ++j) {
                r.canon = canonical(instances + (i * NP + j) * 4);
                if (r.canon) memcpy(im.data() + 4 * j, pzh::from_raw(instances + (i * NP + j) * 4).v, 32);
            }
            tr.common_scalars(im.data(), NP);
        }
        tr.common_points(c, s.A + s.Lk);
        tr.squeeze("theta");
        tr.common_points(c + 8ull * c_ap, 2 * s.Lk);
        r.beta = tr.squeeze("beta");
        r.gamma = tr.squeeze("gamma");
        tr.common_points(c + 8ull * c_pz, s.S + s.Lk + 1);
        r.y = tr.squeeze("y");
        tr.common_points(c + 8ull * c_h, 3);
        r.x = tr.squeeze("x");
        tr.common_scalars(e, s.n_ev - 1);   // h(x), the last element, is the verifier's to compute
        r.sy = tr.squeeze("sh_y");
        r.sv = tr.squeeze("sh_v");
        tr.common_points(c + 8ull * (s.n_own - 2), 1);
        r.su = tr.squeeze("sh_u");
        for (size_t j = 0; j < s.n_ev && r.canon; ++j) r.canon = canonical(e + 4 * j);
        const Fr x = r.x;
        pts[i] = {x, pzh::mul(x, w), pzh::mul(x, pzh::mul(w, w)), pzh::mul(x, pzh::pow_u64(w, 3)), pzh::mul(x, w_u), pzh::mul(x, w_m1)};
        r.inv0 = inv.size();
        inv.push_back(sub(pzh::pow_u64(x, n), one));                // x^n - 1
        Fr wi = one;
        inv.push_back(pzh::mul(nf, sub(x, wi)));                     // l_0
        wi = w_u;
        for (uint32_t b = 0; b <= vk->bf; ++b) {                     // l_last, then the blinding rows
            inv.push_back(pzh::mul(nf, sub(x, wi)));
            wi = pzh::mul(wi, w);
        }
        for (uint32_t k = 0; k < s.n_sets; ++k)                      // the interpolation's denominators
            for (uint32_t q = 0; q < s.set_npts[k]; ++q) {
                Fr d = one;
                for (uint32_t j = 0; j < s.set_npts[k]; ++j)
                    if (j != q) d = pzh::mul(d, sub(pts[i][vk->set_pts[k][q]], pts[i][vk->set_pts[k][j]]));
                inv.push_back(d);
            }
    }
    std::vector<Fr> inv_in = inv;
    batch_invert(inv);

    // 2. the per-proof scalar blocks
    std::vector<uint64_t> pp(B * 4 * VP_COUNT, 0);
    std::vector<char> good(B);
    for (size_t i = 0; i < B; ++i) {
        const Replay& r = rp[i];
        const std::vector<Fr>& P = pts[i];
        bool nz = true;
        size_t cnt = 2 + (vk->bf + 1);
        for (uint32_t k = 0; k < s.n_sets; ++k) cnt += s.set_npts[k];
        for (size_t j = 0; j < cnt; ++j) nz = nz && !is_zero(inv_in[r.inv0 + j]);
        good[i] = r.canon && nz;
        Fr* v = (Fr*)(pp.data() + i * 4 * VP_COUNT);
        const Fr* I = inv.data() + r.inv0;
        const Fr xn1 = inv_in[r.inv0];
        v[VP_BETA] = r.beta;
        v[VP_GAMMA] = r.gamma;
        v[VP_Y] = r.y;
        v[VP_BX] = pzh::mul(r.beta, r.x);
        v[VP_XN] = pzh::pow_u64(r.x, n);
        v[VP_SY] = r.sy;
        v[VP_INV] = I[0];
        v[VP_L0] = pzh::mul(xn1, I[1]);
        Fr wi = w_u, blind = {{0, 0, 0, 0}};
        v[VP_LLAST] = pzh::mul(pzh::mul(xn1, wi), I[2]);
        for (uint32_t b = 1; b <= vk->bf; ++b) {
            wi = pzh::mul(wi, w);
            blind = pzh::add(blind, pzh::mul(pzh::mul(xn1, wi), I[2 + b]));
        }
        v[VP_LACT] = sub(sub(one, v[VP_LLAST]), blind);
        Fr zt = one;
        for (int t = 0; t < 6; ++t) zt = pzh::mul(zt, sub(r.su, P[t]));
        size_t d = 3 + vk->bf;
        Fr svk = one, z0 = one;
        for (uint32_t k = 0; k < s.n_sets; ++k) {
            Fr zk = one;
            for (uint32_t t = 0; t < 6; ++t) {
                bool in = false;
                for (uint32_t q = 0; q < s.set_npts[k]; ++q) in = in || vk->set_pts[k][q] == t;
                if (!in) zk = pzh::mul(zk, sub(r.su, P[t]));
            }
            if (k == 0) z0 = zk;
            v[VP_COEF + k] = pzh::mul(svk, zk);
            svk = pzh::mul(svk, r.sv);
            for (uint32_t q = 0; q < s.set_npts[k]; ++q) {
                Fr num = one;
                for (uint32_t j = 0; j < s.set_npts[k]; ++j)
                    if (j != q) num = pzh::mul(num, sub(r.su, P[vk->set_pts[k][j]]));
                v[VP_LAG + 4 * k + q] = pzh::mul(num, I[d++]);
            }
        }
        v[VP_W1A] = pzh::neg(zt);
        v[VP_W2A] = pzh::mul(z0, r.su);
        v[VP_W2B] = pzh::neg(z0);
    }

    // 3. the device: evaluations, scalar blocks, bases [fixed | sigma | g0 | commitments of proof 0, 1, ...]
    const size_t nb = s.n_vkb + B * s.n_own;
    std::vector<uint64_t> h_ev(B * ew), h_com(B * cw);
    for (size_t i = 0; i < B; ++i) {
        memcpy(h_com.data() + i * cw, proofs + i * pw, cw * 8);
        memcpy(h_ev.data() + i * ew, proofs + i * pw + cw, ew * 8);
    }
    Dev d_ev(ctx), d_pp(ctx), d_h(ctx), d_id(ctx), d_own(ctx), d_vksc(ctx), d_gp(ctx), d_bases(ctx);
    d_ev.alloc(h_ev.size() * 8);
    d_pp.alloc(pp.size() * 8);
    d_h.alloc(B * 32);
    d_id.alloc(B * 4);
    d_own.alloc(B * 2 * s.n_own * 32);
    d_vksc.alloc(B * s.n_vkb * 32);
    d_gp.alloc(B * PZ_VSETS_MAX * 32);
    d_bases.alloc(nb * 64);
    ck(pz_upload(ctx, d_ev.d, h_ev.data(), h_ev.size() * 8));
    ck(pz_upload(ctx, d_pp.d, pp.data(), pp.size() * 8));
    ck(pz_dev_memset(ctx, d_own.d, 0, B * 2 * s.n_own * 32));
    ck(pz_dev_memset(ctx, d_gp.d, 0, B * PZ_VSETS_MAX * 32));
    ck(pz_dev_copy(ctx, d_bases.d, vk->d_vkb, s.n_vkb * 64ull));
    ck(pz_upload(ctx, d_bases.p() + 8ull * s.n_vkb, h_com.data(), h_com.size() * 8));
    // the caller's commitments come unchecked: one launch holds every one to what the wire decoder asks of a point (the identity, or
    // canonical coordinates on the curve); a proof with a commitment that fails is refused, the others are judged without it
    Dev d_cfl(ctx);
    d_cfl.alloc(B * 4);
    ck(pz_g1_check_groups_launch(ctx, d_bases.p() + 8ull * s.n_vkb, B, s.n_own, d_cfl.p<int32_t>()));
    Dev d_inst(ctx), d_x(ctx), d_fl(ctx);
    std::vector<int32_t> iflags(B, 0);
    if (NP) {   // the instance column at every proof's x, straight into its scalar block
        std::vector<uint64_t> xs(B * 4);
        for (size_t i = 0; i < B; ++i) memcpy(xs.data() + 4 * i, rp[i].x.v, 32);
        const Fr n_inv = pzh::inv(nf);
        d_inst.alloc(B * NP * 32);
        d_x.alloc(B * 32);
        d_fl.alloc(B * 4);
        ck(pz_upload(ctx, d_inst.d, instances, B * NP * 32));
        ck(pz_upload(ctx, d_x.d, xs.data(), B * 32));
        ck(pz_instance_eval_launch(ctx, vk->k, w.v, n_inv.v, d_inst.p(), NP, B, d_x.p(), 4, d_pp.p() + 4 * VP_INST, 4 * VP_COUNT, d_fl.p<int32_t>()));
    }
    ck(pz_verify_terms_launch(ctx, s, B, (const uint32_t*)vk->d_members, d_ev.p(), d_pp.p(), (const uint64_t*)vk->d_delta, d_h.p(),
                              d_id.p<int32_t>(), d_own.p(), d_vksc.p(), d_gp.p()));
    std::vector<int32_t> ident(B), cflags(B);
    std::vector<uint64_t> hx(B * 4);
    ck(pz_download(ctx, ident.data(), d_id.d, B * 4));
    ck(pz_download(ctx, cflags.data(), d_cfl.d, B * 4));
    ck(pz_download(ctx, hx.data(), d_h.d, B * 32));
    if (NP) {
        ck(pz_download(ctx, iflags.data(), d_fl.d, B * 4));
        for (size_t i = 0; i < B; ++i) good[i] = good[i] && iflags[i] == 0;   // x on the domain, or a value >= r
    }
    if (h_evals) memcpy(h_evals, hx.data(), B * 32);
    bool all_ident = true;
    for (size_t i = 0; i < B; ++i) {
        good[i] = good[i] && cflags[i] == 0 && (ident[i] == 1 || !stated_h);
        all_ident = all_ident && good[i];
    }
    uint32_t nwin = 0;

    // 4. happy path: one random fold, one MSM, one check
    if (all_ident && !ab_affine) {
        std::vector<uint64_t> rw(B * 4);
        if (!os_random(rw.data(), rw.size() * 8)) throw Fail{PZ_ERR_INTERNAL};
        for (size_t i = 0; i < B; ++i) {
            rw[4 * i + 3] &= 0x0fffffffffffffffULL;   // a 252-bit weight, below r
            const Fr m = pzh::from_raw(rw.data() + 4 * i);
            memcpy(rw.data() + 4 * i, m.v, 32);
        }
        Dev d_r(ctx), d_cols(ctx), d_jac(ctx), d_g1(ctx), d_g2(ctx), d_ok(ctx);
        d_r.alloc(B * 32);
        d_cols.alloc(2 * nb * 32);
        d_jac.alloc(2 * 96);
        d_g1.alloc(2 * 64);
        d_g2.alloc(2 * 128);
        d_ok.alloc(4);
        ck(pz_upload(ctx, d_r.d, rw.data(), B * 32));
        ck(pz_verify_fold_launch(ctx, s, B, 0, d_r.p(), d_vksc.p(), d_gp.p(), d_own.p(), d_cols.p()));
        BasesGuard tb{ctx};
        ck(pz_bases_load_g1(ctx, d_bases.p(), nb, 1, 0, &tb.b));
        ck(pz_bases_info(tb.b, nullptr, nullptr, &nwin));
        ck(pz_msm_g1_dev(ctx, tb.b, d_cols.p(), 2, nb, 4 * nb, 0, nwin, d_jac.p()));
        uint64_t jac[24], aff[16];
        ck(pz_download(ctx, jac, d_jac.d, sizeof jac));
        ck(pz_g1_normalize(ctx, jac, 2, aff));
        ck(pz_upload(ctx, d_g1.d, aff, sizeof aff));
        ck(pz_upload(ctx, d_g2.d, vk->g2, sizeof vk->g2));
        ck(pz_pairing_check_dev(ctx, d_g1.p(), d_g2.p(), 1, 2, d_ok.p<int32_t>()));
        int32_t ok = 0;
        ck(pz_download(ctx, &ok, d_ok.d, 4));
        if (ok == 1) {
            for (size_t i = 0; i < B; ++i) verdicts[i] = 1;
            *all_ok = 1;
            return;
        }
    }

    // 5. per proof: the vk part of every proof in one B-column MSM, the own part per proof, B checks in one launch
    Dev d_jvk(ctx), d_jown(ctx), d_g1(ctx), d_g2(ctx), d_ok(ctx);
    d_jvk.alloc(B * 96);
    d_jown.alloc(B * 2 * 96);
    d_g1.alloc(B * 2 * 64);
    d_g2.alloc(B * 2 * 128);
    d_ok.alloc(B * 4);
    ck(pz_verify_fold_launch(ctx, s, B, 1, nullptr, d_vksc.p(), d_gp.p(), d_own.p(), nullptr));
    ck(pz_bases_info(vk->t_vk, nullptr, nullptr, &nwin));
    ck(pz_msm_g1_dev(ctx, vk->t_vk, d_vksc.p(), B, s.n_vkb, 4ull * s.n_vkb, 0, nwin, d_jvk.p()));
    for (size_t i = 0; i < B; ++i) {
        BasesGuard tb{ctx};
        ck(pz_bases_load_g1(ctx, d_bases.p() + 8ull * (s.n_vkb + i * s.n_own), s.n_own, 1, 0, &tb.b));
        ck(pz_bases_info(tb.b, nullptr, nullptr, &nwin));
        ck(pz_msm_g1_dev(ctx, tb.b, d_own.p() + 8ull * s.n_own * i, 2, s.n_own, 4ull * s.n_own, 0, nwin, d_jown.p() + 24 * i));
    }
    std::vector<uint64_t> jvk(B * 12), jown(B * 24), jab(B * 24), aff(B * 16), g2s(B * 32);
    ck(pz_download(ctx, jvk.data(), d_jvk.d, B * 96));
    ck(pz_download(ctx, jown.data(), d_jown.d, B * 192));
    for (size_t i = 0; i < B; ++i) {
        uint64_t two[24];
        memcpy(two, jvk.data() + 12 * i, 96);
        memcpy(two + 12, jown.data() + 24 * i, 96);
        ck(pz_g1_sum(ctx, two, 2, jab.data() + 24 * i));                      // A = vk part + own part
        memcpy(jab.data() + 24 * i + 12, jown.data() + 24 * i + 12, 96);    // B: own part only
        memcpy(g2s.data() + 32 * i, vk->g2, 256);
    }
    ck(pz_g1_normalize(ctx, jab.data(), 2 * B, aff.data()));
    ck(pz_upload(ctx, d_g1.d, aff.data(), aff.size() * 8));
    ck(pz_upload(ctx, d_g2.d, g2s.data(), g2s.size() * 8));
    ck(pz_pairing_check_dev(ctx, d_g1.p(), d_g2.p(), B, 2, d_ok.p<int32_t>()));
    std::vector<int32_t> ok(B);
    ck(pz_download(ctx, ok.data(), d_ok.d, B * 4));
    if (ab_affine) memcpy(ab_affine, aff.data(), B * 128);
    int all = 1;
    for (size_t i = 0; i < B; ++i) {
        verdicts[i] = good[i] && ok[i] == 1 ? 1 : 0;
        all = all && verdicts[i];
    }
    *all_ok = all;
}

// B proofs between host wire bytes and host words through the device codec (pz_wire.hip); decode also brings each proof's status back
void wire_codec(pz_vk* vk, size_t B, bool decode, uint8_t* bytes, uint64_t* words, int32_t* status) {
    pz_ctx* ctx = vk->ctx;
    const pz_vshape& s = vk->s;
    const size_t wire = 32ull * (s.n_own + s.n_ev - 1), pw = 8ull * s.n_own + 4ull * s.n_ev;
    Dev d_bytes(ctx), d_words(ctx), d_st(ctx);
    d_bytes.alloc(B * wire);
    d_words.alloc(B * pw * 8);
    d_st.alloc((B * (s.n_own + s.n_ev) + B) * 4);
    int32_t* d_elem = d_st.p<int32_t>();
    int32_t* d_proof = d_elem + B * (s.n_own + s.n_ev);
    if (decode) {
        ck(pz_upload(ctx, d_bytes.d, bytes, B * wire));
        ck(pz_wire_proofs_launch(ctx, s, B, 1, d_bytes.p<uint8_t>(), d_words.p(), d_elem, d_proof));
        ck(pz_download(ctx, words, d_words.d, B * pw * 8));
        ck(pz_download(ctx, status, d_proof, B * 4));
    } else {
        ck(pz_upload(ctx, d_words.d, words, B * pw * 8));
        ck(pz_wire_proofs_launch(ctx, s, B, 0, d_bytes.p<uint8_t>(), d_words.p(), nullptr, nullptr));
        ck(pz_download(ctx, bytes, d_bytes.d, B * wire));
    }
}

bool all_zero(const uint64_t* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (v[i]) return false;
    return true;
}

}  // namespace

bool pz_os_random(void* buf, size_t n) { return os_random(buf, n); }

namespace {
int vk_create(pz_ctx* ctx, size_t n_instance, size_t n_public, uint32_t k, uint32_t blinding_factors, size_t n_adv, size_t n_lk, const uint64_t* fixed_affine,
                            const uint64_t* sigma_affine, const uint64_t g0_affine[8], const uint64_t g2[16], const uint64_t s_g2[16],
                            pz_vk** out) {
    if (!ctx || !fixed_affine || !sigma_affine || !g0_affine || !g2 || !s_g2 || !out) return PZ_ERR_INVALID;
    *out = nullptr;
    if (k < 4 || k > 24 || !n_adv || !n_lk || (uint64_t)blinding_factors + 2 > (1ull << k)) return PZ_ERR_INVALID;
    if (n_instance > 1 || (n_instance ? n_public == 0 || n_public + blinding_factors + 1 > (1ull << k) : n_public != 0)) return PZ_ERR_INVALID;
    if (n_adv + n_lk >= (1u << 24)) return PZ_ERR_UNSUPPORTED;   // offsets and slots are 30-bit on the device
    if (all_zero(g2, 16) || all_zero(s_g2, 16) || all_zero(g0_affine, 8)) return PZ_ERR_INVALID;
    PZ_ENTER(ctx);
    pz_vk* vk = new (std::nothrow) pz_vk;
    if (!vk) return PZ_ERR_OOM;
    vk->ctx = ctx;
    vk->k = k;
    vk->bf = blinding_factors;
    const int rc = guarded([&] {
        std::vector<uint32_t> mem;
        make_shape(n_adv, n_lk, n_instance, *vk, mem);
        vk->n_public = n_public;
        const pz_vshape& s = vk->s;
        memcpy(vk->g2, g2, 128);
        memcpy(vk->g2 + 16, s_g2, 128);
        std::vector<uint64_t> vkb(8ull * s.n_vkb);
        memcpy(vkb.data(), fixed_affine, 64ull * s.F);
        memcpy(vkb.data() + 8ull * s.F, sigma_affine, 64ull * s.m);
        memcpy(vkb.data() + 8ull * (s.F + s.m), g0_affine, 64);
        vk->commitments.assign(vkb.begin(), vkb.begin() + 8ull * (s.F + s.m));
        std::vector<uint64_t> delta(4ull * s.m);
        const Fr dl = pzh::delta();
        Fr dc = pzh::FR_ONE;
        for (uint32_t c = 0; c < s.m; ++c) {
            memcpy(delta.data() + 4ull * c, dc.v, 32);
            dc = pzh::mul(dc, dl);
        }
        ck(pz_dev_alloc(ctx, vkb.size() * 8, &vk->d_vkb));
        ck(pz_dev_alloc(ctx, delta.size() * 8, &vk->d_delta));
        ck(pz_dev_alloc(ctx, mem.size() * 4, &vk->d_members));
        ck(pz_upload(ctx, vk->d_vkb, vkb.data(), vkb.size() * 8));
        ck(pz_upload(ctx, vk->d_delta, delta.data(), delta.size() * 8));
        ck(pz_upload(ctx, vk->d_members, mem.data(), mem.size() * 4));
        ck(pz_bases_load_g1(ctx, (const uint64_t*)vk->d_vkb, s.n_vkb, 1, 0, &vk->t_vk));
        ck(pz_sync(ctx));
    });
    if (rc != PZ_OK) {
        pz_vk_free(vk);
        return rc;
    }
    *out = vk;
    return PZ_OK;
}

}   // namespace

extern "C" int pz_vk_create(pz_ctx* ctx, uint32_t k, uint32_t blinding_factors, size_t n_adv, size_t n_lk, const uint64_t* fixed_affine,
                            const uint64_t* sigma_affine, const uint64_t g0_affine[8], const uint64_t g2[16], const uint64_t s_g2[16],
                            pz_vk** out) {
    return vk_create(ctx, 0, 0, k, blinding_factors, n_adv, n_lk, fixed_affine, sigma_affine, g0_affine, g2, s_g2, out);
}
// the same for a key with the optional instance column: sigma_affine is (m + n_instance) x 8
extern "C" int pz_vk_create_pub(pz_ctx* ctx, uint32_t k, uint32_t blinding_factors, size_t n_adv, size_t n_lk, size_t n_instance, size_t n_public,
                                const uint64_t* fixed_affine, const uint64_t* sigma_affine, const uint64_t g0_affine[8], const uint64_t g2[16],
                                const uint64_t s_g2[16], pz_vk** out) {
    return vk_create(ctx, n_instance, n_public, k, blinding_factors, n_adv, n_lk, fixed_affine, sigma_affine, g0_affine, g2, s_g2, out);
}

extern "C" int pz_vk_info(const pz_vk* vk, size_t* commitment_words, size_t* evals_words) {
    if (!vk) return PZ_ERR_INVALID;
    if (commitment_words) *commitment_words = 8ull * vk->s.n_own;
    if (evals_words) *evals_words = 4ull * vk->s.n_ev;
    return PZ_OK;
}

namespace {
int verify_batch(pz_vk* vk, const uint64_t* instances, size_t n_public, const uint64_t* proofs, size_t n_proofs, const uint8_t* seeds, const size_t* seed_offsets,
                               int32_t* verdicts, uint64_t* h_evals, uint64_t* ab_affine, int* all_ok) {
    if (!vk || !proofs || !n_proofs || !seed_offsets || !verdicts || !all_ok) return PZ_ERR_INVALID;
    if (n_public != vk->n_public || (n_public && !instances)) return PZ_ERR_INVALID;   // (an instance key through the old entry point too)
    if (n_proofs > (1u << 20)) return PZ_ERR_UNSUPPORTED;
    for (size_t i = 0; i < n_proofs; ++i)
        if (seed_offsets[i + 1] < seed_offsets[i]) return PZ_ERR_INVALID;
    if (seed_offsets[n_proofs] > seed_offsets[0] && !seeds) return PZ_ERR_INVALID;
    pz_ctx* ctx = vk->ctx;
    PZ_ENTER(ctx);
    *all_ok = 0;
    for (size_t i = 0; i < n_proofs; ++i) verdicts[i] = 0;
    return guarded([&] { verify(vk, proofs, n_proofs, seeds, seed_offsets, verdicts, h_evals, ab_affine, all_ok, true, instances); });
}

}   // namespace

extern "C" int pz_verify_batch(pz_vk* vk, const uint64_t* proofs, size_t n_proofs, const uint8_t* seeds, const size_t* seed_offsets,
                               int32_t* verdicts, uint64_t* h_evals, uint64_t* ab_affine, int* all_ok) {
    return verify_batch(vk, nullptr, 0, proofs, n_proofs, seeds, seed_offsets, verdicts, h_evals, ab_affine, all_ok);
}
// instances: n_proofs x n_public x 4 canonical words (host).  A value >= r: verdict 0 for that proof, the others are judged without it
extern "C" int pz_verify_batch_pub(pz_vk* vk, const uint64_t* instances, size_t n_public, const uint64_t* proofs, size_t n_proofs,
                                   const uint8_t* seeds, const size_t* seed_offsets, int32_t* verdicts, uint64_t* h_evals, uint64_t* ab_affine,
                                   int* all_ok) {
    return verify_batch(vk, instances, n_public, proofs, n_proofs, seeds, seed_offsets, verdicts, h_evals, ab_affine, all_ok);
}

extern "C" int pz_proof_wire_bytes(const pz_vk* vk, size_t* bytes) {
    if (!vk || !bytes) return PZ_ERR_INVALID;
    *bytes = 32ull * (vk->s.n_own + vk->s.n_ev - 1);
    return PZ_OK;
}

extern "C" int pz_proof_encode(pz_vk* vk, const uint64_t* proofs_words, size_t n_proofs, uint8_t* out_bytes) {
    if (!vk || !proofs_words || !n_proofs || !out_bytes) return PZ_ERR_INVALID;
    if (n_proofs > (1u << 20)) return PZ_ERR_UNSUPPORTED;
    pz_ctx* ctx = vk->ctx;
    PZ_ENTER(ctx);
    return guarded([&] { wire_codec(vk, n_proofs, false, out_bytes, const_cast<uint64_t*>(proofs_words), nullptr); });
}

extern "C" int pz_proof_decode(pz_vk* vk, const uint8_t* bytes, size_t n_proofs, uint64_t* out_words, int32_t* status) {
    if (!vk || !bytes || !n_proofs || !out_words || !status) return PZ_ERR_INVALID;
    if (n_proofs > (1u << 20)) return PZ_ERR_UNSUPPORTED;
    pz_ctx* ctx = vk->ctx;
    PZ_ENTER(ctx);
    return guarded([&] { wire_codec(vk, n_proofs, true, const_cast<uint8_t*>(bytes), out_words, status); });
}

namespace {
int verify_batch_bytes(pz_vk* vk, const uint64_t* instances, size_t n_public, const uint8_t* bytes, size_t n_proofs, const uint8_t* seeds, const size_t* seed_offsets,
                                     int32_t* verdicts, uint64_t* h_evals, uint64_t* ab_affine, int* all_ok) {
    if (!vk || !bytes || !n_proofs || !seed_offsets || !verdicts || !all_ok) return PZ_ERR_INVALID;
    if (n_public != vk->n_public || (n_public && !instances)) return PZ_ERR_INVALID;
    if (n_proofs > (1u << 20)) return PZ_ERR_UNSUPPORTED;
    for (size_t i = 0; i < n_proofs; ++i)
        if (seed_offsets[i + 1] < seed_offsets[i]) return PZ_ERR_INVALID;
    if (seed_offsets[n_proofs] > seed_offsets[0] && !seeds) return PZ_ERR_INVALID;
    pz_ctx* ctx = vk->ctx;
    PZ_ENTER(ctx);
    *all_ok = 0;
    for (size_t i = 0; i < n_proofs; ++i) verdicts[i] = 0;
    if (h_evals) memset(h_evals, 0, n_proofs * 32);
    if (ab_affine) memset(ab_affine, 0, n_proofs * 128);
    return guarded([&] {
        const size_t pw = 8ull * vk->s.n_own + 4ull * vk->s.n_ev;
        std::vector<uint64_t> words(n_proofs * pw);
        std::vector<int32_t> st(n_proofs);
        wire_codec(vk, n_proofs, true, const_cast<uint8_t*>(bytes), words.data(), st.data());
        // the proofs that decoded, moved together with their seeds: a refused proof's words never reach verify()
        std::vector<size_t> live, off(1, 0);
        std::vector<uint8_t> sd;
        std::vector<uint64_t> inst;   // the live proofs' statements, moved together like their seeds
        for (size_t i = 0; i < n_proofs; ++i) {
            if (st[i] != 0) continue;
            if (live.size() != i) memmove(words.data() + live.size() * pw, words.data() + i * pw, pw * 8);
            live.push_back(i);
            if (n_public) inst.insert(inst.end(), instances + i * n_public * 4, instances + (i + 1) * n_public * 4);
            if (seed_offsets[i + 1] > seed_offsets[i]) sd.insert(sd.end(), seeds + seed_offsets[i], seeds + seed_offsets[i + 1]);
            off.push_back(sd.size());
        }
        const size_t L = live.size();
        if (!L) return;
        std::vector<int32_t> v(L, 0);
        std::vector<uint64_t> hx(h_evals ? L * 4 : 0), ab(ab_affine ? L * 16 : 0);
        int ok = 0;
        verify(vk, words.data(), L, sd.data(), off.data(), v.data(), h_evals ? hx.data() : nullptr, ab_affine ? ab.data() : nullptr, &ok,
               false, n_public ? inst.data() : nullptr);
        for (size_t j = 0; j < L; ++j) {
            verdicts[live[j]] = v[j];
            if (h_evals) memcpy(h_evals + 4 * live[j], hx.data() + 4 * j, 32);
            if (ab_affine) memcpy(ab_affine + 16 * live[j], ab.data() + 16 * j, 128);
        }
        *all_ok = ok && L == n_proofs;
    });
}

}   // namespace

extern "C" int pz_verify_batch_bytes(pz_vk* vk, const uint8_t* bytes, size_t n_proofs, const uint8_t* seeds, const size_t* seed_offsets,
                                     int32_t* verdicts, uint64_t* h_evals, uint64_t* ab_affine, int* all_ok) {
    return verify_batch_bytes(vk, nullptr, 0, bytes, n_proofs, seeds, seed_offsets, verdicts, h_evals, ab_affine, all_ok);
}
extern "C" int pz_verify_batch_bytes_pub(pz_vk* vk, const uint64_t* instances, size_t n_public, const uint8_t* bytes, size_t n_proofs,
                                         const uint8_t* seeds, const size_t* seed_offsets, int32_t* verdicts, uint64_t* h_evals,
                                         uint64_t* ab_affine, int* all_ok) {
    return verify_batch_bytes(vk, instances, n_public, bytes, n_proofs, seeds, seed_offsets, verdicts, h_evals, ab_affine, all_ok);
}

// the key's digest and the opt-in binding of every verification to it (host/key_digest.hpp)
extern "C" int pz_key_digest(uint32_t k, uint32_t blinding_factors, size_t n_adv, size_t n_lk, size_t n_instance, size_t n_public,
                             const uint64_t* fixed_affine, const uint64_t* sigma_affine, uint8_t out[64]) {
    if (!fixed_affine || !sigma_affine || !out) return PZ_ERR_INVALID;
    if (!n_instance && n_public) return PZ_ERR_INVALID;
    pzh::key_digest(k, blinding_factors, n_adv, n_lk, n_instance, n_public, fixed_affine, sigma_affine, out);
    return PZ_OK;
}

extern "C" int pz_vk_digest(const pz_vk* vk, uint8_t out[64]) {
    if (!vk || !out) return PZ_ERR_INVALID;
    memcpy(out, vk_digest(const_cast<pz_vk*>(vk)), pzh::KEY_DIGEST_BYTES);
    return PZ_OK;
}

extern "C" int pz_vk_bind(pz_vk* vk, int on) {
    if (!vk) return PZ_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(vk->ctx->mu);   // not under a verification in flight on this key's context
    vk->bound = on != 0;
    return PZ_OK;
}

extern "C" int pz_vk_is_bound(const pz_vk* vk, int* on) {
    if (!vk || !on) return PZ_ERR_INVALID;
    *on = vk->bound ? 1 : 0;
    return PZ_OK;
}

extern "C" int pz_vk_free(pz_vk* vk) {
    if (!vk) return PZ_ERR_INVALID;
    pz_ctx* ctx = vk->ctx;
    if (vk->t_vk) pz_bases_free(ctx, vk->t_vk);
    for (void* d : {vk->d_vkb, vk->d_delta, vk->d_members})
        if (d) pz_dev_free(ctx, d);
    delete vk;
    return PZ_OK;
}
