// The packed ballot's host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierChip::pballot, paillier_pballot_test,
// synthesize_pballot_circuit, pz::pballot_bases, pz::unpack_tally) on seeded inputs, over the C ABI alone and
// self-checking with host/biguint.hpp: the slot bases read from one device trace equal g^(2^(j w)) mod n^2 in BigUint arithmetic; the
// tape's operation order is the circuit's, its cell totals are pz_pballot_cells, its records are pz_paillier_pballot's, every ciphertext is
// g^M hs^s mod n^2 with M the packed plaintext, the device expansion of the tape holds the statement n | hs | G_0 .. G_{K-1} | c_1 .. c_R
// | S_1 .. S_R at pz_pballot_public_cells and every assert_equal_fresh's bit -- 1 for the honest results, 0 for a wrong one.
// `--host-only` stops before anything needs a device.
#include <cstdio>
#include <cstring>
#include <random>

#include <hip/hip_runtime_api.h>

#include "../../paillier_halo2_amd/host/paillier_chip.hpp"

using namespace pz;

static std::mt19937_64 rng(0x9ba110);
static BigUint gen_biguint(unsigned bits) {
    std::vector<uint64_t> v((bits + 63) / 64);
    for (auto& w : v) w = rng();
    if (bits % 64) v.back() &= (1ull << (bits % 64)) - 1;
    return BigUint::from_limbs(v.data(), v.size());
}
static BigUint gen_modulus(unsigned enc_bits) {   // a full-size odd modulus
    BigUint n = gen_biguint(enc_bits).low_bits(enc_bits - 1) + (BigUint(1) << (enc_bits - 1));
    if (!n.bit(0)) n = n + BigUint(1);
    return n;
}
static BigUint pow_mod(const BigUint& base, const BigUint& e, const BigUint& m) {   // square-and-multiply, LSB first
    BigUint acc(1), sq = base % m;
    for (size_t j = 0; j < e.bits(); ++j) {
        if (e.bit(j)) acc = acc * sq % m;
        sq = sq * sq % m;
    }
    return acc;
}

static int failures = 0;
#define CHECK(cond, what)                                          \
    do {                                                           \
        if (!(cond)) { std::printf("FAIL %s\n", what); ++failures; } \
        else std::printf("ok   %s\n", what);                       \
    } while (0)

// whether advice cell `cell` (Montgomery form on the device) holds the integer `want`
static bool cell_is(Context& ctx, const uint64_t* d_adv, uint64_t cell, const BigUint& want) {
    uint64_t got[4], *d_tmp = nullptr;
    if (hipMalloc((void**)&d_tmp, 32) != hipSuccess) return false;
    bool ok = hipMemcpy(d_tmp, d_adv + 4 * cell, 32, hipMemcpyDeviceToDevice) == hipSuccess &&
              pz_fr_convert_dev(ctx.raw(), d_tmp, 1, 0) == PZ_OK && pz_sync(ctx.raw()) == PZ_OK &&
              hipMemcpy(got, d_tmp, 32, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d_tmp);
    return ok && BigUint::from_limbs(got, 4) == want;
}

static void test_pballot(unsigned enc_bits, unsigned limb_bits, unsigned lookup_bits, unsigned Rn, unsigned K, unsigned m_bits, unsigned w,
                         unsigned s_limbs) {
    static const uint64_t ONE[4] = {0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL};
    Context ctx(0);
    RangeChip range{lookup_bits};
    BigUintChip bchip = BigUintChip::construct(&range, limb_bits);
    PaillierChip pchip = PaillierChip::construct(&bchip, enc_bits);
    const BigUint n = gen_modulus(enc_bits), n2 = n * n, g = n + BigUint(1);
    const unsigned s_bits = s_limbs * limb_bits, sw = (s_bits + 63) / 64;
    BigUint x;
    do x = gen_biguint(enc_bits - 1);
    while (x < BigUint(2) || BigUint::gcd(x, n) != BigUint(1));
    const BigUint hs = djn_generator(ctx, pchip, n, [&](const BigUint&) { return x; }).unwrap();
    // the slot bases from ONE device trace, against BigUint arithmetic
    const std::vector<BigUint> gs = pballot_bases(ctx, n, g, K, w).unwrap();
    bool bases_ok = gs.size() == K;
    for (unsigned j = 0; bases_ok && j < K; ++j) bases_ok = gs[j] == pow_mod(g, BigUint(1) << ((size_t)j * w), n2);
    CHECK(bases_ok, "pballot_bases: G_j == g^(2^(j w)) mod n^2");
    const uint64_t vmax = m_bits == 64 ? ~0ull : (1ull << m_bits) - 1;
    const unsigned L64 = (2 * enc_bits + 63) / 64, wn = (enc_bits + 63) / 64;
    const std::vector<uint64_t> nw = n.to_limbs(wn);
    std::vector<std::vector<uint64_t>> vs(Rn);
    std::vector<BigUint> ss, res, totals;
    const BigUint s_all = (BigUint(1) << s_bits) - BigUint(1);
    bool unpacks = true;
    for (unsigned i = 0; i < Rn; ++i) {
        BigUint M(0), total(0);
        for (unsigned j = 0; j < K; ++j) {
            const unsigned t = i * K + j;
            vs[i].push_back(t == 0 ? vmax : t == 1 ? 0 : t == 2 ? 1ull << (m_bits - 1) : rng() & vmax);   // all ones, zero, a lone top bit
            M = M + (BigUint(vs[i][j]) << ((size_t)j * w));
            total = total + BigUint(vs[i][j]);
        }
        ss.push_back(i == 0 ? BigUint(1) << (s_bits - 1) : i == 1 ? s_all : gen_biguint(s_bits));   // a lone top bit, all ones, random
        res.push_back(pow_mod(g, M, n2) * pow_mod(hs, ss[i], n2) % n2);
        totals.push_back(total);
        const std::vector<BigUint> back = unpack_tally(M, K, w).unwrap();
        for (unsigned j = 0; j < K; ++j) unpacks = unpacks && back[j] == BigUint(vs[i][j]);
    }
    CHECK(unpacks && !unpack_tally(BigUint(1) << ((size_t)K * w), K, w).ok, "unpack_tally inverts the packing and refuses an M of more than K w bits");
    paillier_pballot_test(ctx, range, PaillierPBallotInput{limb_bits, enc_bits, m_bits, s_limbs, n, hs, gs, vs, ss, res});   // throws on any mismatch
    const size_t per = 2 * (size_t)m_bits * K + 2 * (size_t)s_bits + K, ns = Rn * per;
    char name[240];
    std::snprintf(name, sizeof name, "paillier_pballot_test enc_bits=%u limb_bits=%u R=%u K=%u b=%u s_limbs=%u: %zu mul_mod steps, %u limbs in %u words",
                  enc_bits, limb_bits, Rn, K, m_bits, s_limbs, ctx.n_steps(), ctx.limbs(), ctx.words());
    CHECK(ctx.n_steps() == ns && ctx.limbs() == 2 * enc_bits / limb_bits && ctx.words() == L64, name);
    // operation order: assign n, hs, K bases, R K load_witness, R sums (K >= 2), R assigns, square, refresh, load_zero, per ciphertext [per
    // slot: const, const, num_to_bits, b x (mul_mod, select), mul_mod | const, const, per limb of s (num_to_bits, W x (mul_mod, select),
    // mul_mod) -- the last of these with the K folds: one record of 1 + K], then per ciphertext assign res, assert.  The tape merges
    // neighbouring mul_mod records: a bit's square_mod and the next bit's mul_mod.
    std::vector<int> want(2 + K, Context::ASSIGN), got;
    want.insert(want.end(), (size_t)Rn * K, Context::LOAD_WITNESS);
    if (K >= 2) want.insert(want.end(), Rn, Context::SUM);
    want.insert(want.end(), Rn, Context::ASSIGN);
    want.insert(want.end(), {Context::SQUARE, Context::REFRESH, Context::CONST_CELL});
    for (unsigned i = 0; i < Rn; ++i) {
        for (unsigned j = 0; j < K; ++j) {
            want.insert(want.end(), {Context::CONST_CELL, Context::CONST_CELL, Context::NUM_TO_BITS});
            for (unsigned t = 0; t < m_bits; ++t) want.insert(want.end(), {Context::MUL_MOD, Context::SELECT});
            want.push_back(Context::MUL_MOD);
        }
        want.insert(want.end(), {Context::CONST_CELL, Context::CONST_CELL});
        for (unsigned li = 0; li < s_limbs; ++li) {
            want.push_back(Context::NUM_TO_BITS);
            for (unsigned t = 0; t < limb_bits; ++t) want.insert(want.end(), {Context::MUL_MOD, Context::SELECT});
            want.push_back(Context::MUL_MOD);
        }
    }
    for (unsigned i = 0; i < Rn; ++i) want.insert(want.end(), {Context::ASSIGN, Context::ASSERT_EQUAL});
    for (auto& o : ctx.ops()) got.push_back((int)o.op);
    CHECK(got == want && ctx.ops()[got.size() - 2 * Rn - 1].count == 1 + K, "operation order of the tape (DESIGN.md section 15.21)");
    const unsigned Ln = enc_bits / limb_bits;
    size_t a = 0, l = 0;
    int rc = pz_pballot_cells(Ln, limb_bits, lookup_bits, Rn, K, m_bits, s_limbs, &a, &l);
    CHECK(rc == PZ_OK && a == ctx.advice_cells() && l == ctx.lookup_cells(), "tape cell totals == pz_pballot_cells");
    // records: the tape is pz_paillier_pballot's records (repacked to the tape's width), ciphertext-major
    const std::vector<uint64_t>& tp = ctx.tape();
    {
        std::vector<uint64_t> hw = hs.to_limbs(2 * wn), gw, vv, sv, rec(ns * 4 * 2 * wn), cv(Rn * 2 * wn);
        for (const BigUint& gj : gs) {
            std::vector<uint64_t> t = gj.to_limbs(2 * wn);
            gw.insert(gw.end(), t.begin(), t.end());
        }
        for (const auto& row : vs) vv.insert(vv.end(), row.begin(), row.end());
        for (const BigUint& s : ss) {
            std::vector<uint64_t> t = s.to_limbs(sw);
            sv.insert(sv.end(), t.begin(), t.end());
        }
        rc = pz_paillier_pballot(ctx.raw(), wn, Rn, K, m_bits, s_bits, nw.data(), hw.data(), gw.data(), vv.data(), sv.data(), rec.data(), ns, cv.data());
        bool same = rc == PZ_OK && tp.size() == ns * 4 * L64;
        for (size_t f = 0; same && f < ns * 4; ++f) same = std::memcmp(tp.data() + f * L64, rec.data() + f * 2 * wn, L64 * 8) == 0;
        for (unsigned i = 0; same && i < Rn; ++i) same = BigUint::from_limbs(cv.data() + i * 2 * wn, 2 * wn) == res[i];
        CHECK(same, "records == pz_paillier_pballot's, ciphertexts == g^M hs^s mod n^2 in BigUint arithmetic");
    }
    bool recs = BigUint::from_limbs(tp.data(), L64) == BigUint(1);
    for (unsigned j = 0; j < K; ++j) recs = recs && BigUint::from_limbs(tp.data() + (2 * (size_t)m_bits * j * 4 + 1) * L64, L64) == gs[j];   // slot j's first sq
    recs = recs && BigUint::from_limbs(tp.data() + (2 * (size_t)m_bits * K * 4 + 1) * L64, L64) == hs;                                     // the hs-chain's
    for (unsigned i = 0; i < Rn; ++i) recs = recs && BigUint::from_limbs(tp.data() + (((size_t)(i + 1) * per - 1) * 4 + 3) * L64, L64) == res[i];
    CHECK(recs, "records: slot j's chain starts from (1, G_j), the hs-chain from hs, every entry's last remainder is its ciphertext");
    uint64_t *d_work = nullptr, *d_mod = nullptr, *d_adv = nullptr, *d_lk = nullptr;
    std::vector<uint64_t> mod = ctx.modulus().to_limbs(ctx.words());
    bool ok = hipMalloc((void**)&d_work, ns * 4 * 2 * wn * 8) == hipSuccess && hipMalloc((void**)&d_mod, mod.size() * 8) == hipSuccess &&
              hipMalloc((void**)&d_adv, a * 32) == hipSuccess && hipMalloc((void**)&d_lk, l * 32 + 32) == hipSuccess;
    ok = ok && hipMemcpy(d_mod, mod.data(), mod.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
    size_t a_res = 0, a_eq = 0;
    ok = ok && pz_op_cells(0, 2 * Ln, limb_bits, lookup_bits, &a_res, nullptr) == PZ_OK && pz_op_cells(5, 2 * Ln, limb_bits, lookup_bits, &a_eq, nullptr) == PZ_OK;
    bool bits_one = ok, statement = ok, wrong_zero = ok;
    if (ok) {
        ok = synthesize_pballot_circuit(ctx, enc_bits, m_bits, s_limbs, n, hs, gs, vs, ss, res, d_work, d_mod, d_adv, d_lk) == PZ_OK &&
             pz_sync(ctx.raw()) == PZ_OK;
        for (unsigned i = 0; ok && i < Rn; ++i) {   // entry i's assert_equal_fresh ends (R - 1 - i) result blocks before the stream's end
            uint64_t last[4];
            ok = hipMemcpy(last, d_adv + 4 * (a - 1 - (size_t)(Rn - 1 - i) * (a_res + a_eq)), 32, hipMemcpyDeviceToHost) == hipSuccess;
            bits_one = bits_one && ok && std::memcmp(last, ONE, 32) == 0;
        }
        // the statement: n | hs | G_0 .. G_{K-1} | c_1 .. c_R | S_1 .. S_R, limb by limb, at the cells pz_pballot_public_cells names
        std::vector<uint64_t> cells(Ln + 2 * Ln * (1 + K + Rn) + Rn);
        size_t npub = 0;
        ok = ok && pz_pballot_public_cells(Ln, limb_bits, lookup_bits, Rn, K, m_bits, s_limbs, cells.data(), cells.size(), &npub) == PZ_OK;
        statement = ok && npub == Ln + (size_t)2 * Ln * (1 + K + Rn) + (K >= 2 ? Rn : 0);
        std::vector<BigUint> want_st;
        auto limbs_of = [&](const BigUint& v, unsigned cnt) {
            for (unsigned j = 0; j < cnt; ++j) want_st.push_back((v >> (j * limb_bits)).low_bits(limb_bits));
        };
        limbs_of(n, Ln);
        limbs_of(hs, 2 * Ln);
        for (const BigUint& gj : gs) limbs_of(gj, 2 * Ln);
        for (const BigUint& c : res) limbs_of(c, 2 * Ln);
        if (K >= 2) want_st.insert(want_st.end(), totals.begin(), totals.end());
        for (size_t i = 0; statement && i < npub; ++i) statement = cell_is(ctx, d_adv, cells[i], want_st[i]);
        std::vector<BigUint> wrong = res;
        wrong.back() = wrong.back() + BigUint(1);
        uint64_t last_bad[4] = {1, 1, 1, 1}, first_ok[4] = {0, 0, 0, 0};
        wrong_zero = ok && synthesize_pballot_circuit(ctx, enc_bits, m_bits, s_limbs, n, hs, gs, vs, ss, wrong, d_work, d_mod, d_adv, d_lk) == PZ_OK &&
                     pz_sync(ctx.raw()) == PZ_OK && hipMemcpy(last_bad, d_adv + 4 * (a - 1), 32, hipMemcpyDeviceToHost) == hipSuccess &&
                     hipMemcpy(first_ok, d_adv + 4 * (a - 1 - (size_t)(Rn - 1) * (a_res + a_eq)), 32, hipMemcpyDeviceToHost) == hipSuccess;
        wrong_zero = wrong_zero && (last_bad[0] | last_bad[1] | last_bad[2] | last_bad[3]) == 0 && (Rn == 1 || std::memcmp(first_ok, ONE, 32) == 0);
    }
    (void)hipFree(d_work); (void)hipFree(d_mod); (void)hipFree(d_adv); (void)hipFree(d_lk);
    CHECK(ok && bits_one, "device expansion of the tape: every assert_equal_fresh == 1");
    CHECK(ok && statement, "the exposed cells hold n | hs | G_0 .. G_{K-1} | c_1 .. c_R | S_1 .. S_R");
    CHECK(ok && wrong_zero, "a wrong last `res` expands to assert_equal_fresh == 0 for that entry alone");
}

static void test_refusals() {
    Context ctx(0);
    RangeChip range{10};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
    const BigUint n = gen_modulus(128);
    auto na = chip.assign_integer(ctx, n, 128).unwrap();
    auto hs = chip.assign_integer(ctx, gen_biguint(250), 256).unwrap();
    auto g0 = chip.assign_integer(ctx, n + BigUint(1), 256).unwrap();
    auto g1 = chip.assign_integer(ctx, gen_biguint(250), 256).unwrap();
    auto s1 = chip.assign_integer(ctx, gen_biguint(60), 64).unwrap();
    auto s2 = chip.assign_integer(ctx, gen_biguint(120), 128).unwrap();
    auto s5 = chip.assign_integer(ctx, gen_biguint(300), 320).unwrap();
    const AssignedWeight v1{1, ctx.load_witness()}, v4{4, ctx.load_witness()};
    using Rows = std::vector<std::vector<AssignedWeight>>;
    CHECK(pc.pballot(ctx, na, hs, {g0, g1}, Rows{{v1, v4}}, {s1}, 2).err.status == PZ_ERR_MESSAGE_RANGE,
          "pballot refuses a value of 2^b (PZ_ERR_MESSAGE_RANGE)");
    CHECK(pc.pballot(ctx, na, hs, {g0}, Rows{{v1}}, {s1}, 0).err.status == PZ_ERR_INVALID &&
              pc.pballot(ctx, na, hs, {g0}, Rows{{v1}}, {s1}, 65).err.status == PZ_ERR_INVALID,
          "pballot refuses b = 0 and b = 65");
    CHECK(pc.pballot(ctx, na, hs, {g0}, Rows{{v1}, {v1}}, {s1}, 2).err.status == PZ_ERR_INVALID, "pballot refuses a missing s");
    CHECK(pc.pballot(ctx, na, hs, {g0}, Rows{}, {}, 2).err.status == PZ_ERR_INVALID, "pballot refuses no ciphertext");
    CHECK(pc.pballot(ctx, na, hs, {}, Rows{{}}, {s1}, 2).err.status == PZ_ERR_INVALID, "pballot refuses no slot");
    CHECK(pc.pballot(ctx, na, hs, {g0, g1}, Rows{{v1}}, {s1}, 2).err.status == PZ_ERR_INVALID, "pballot refuses a row that is not one value per slot");
    CHECK(pc.pballot(ctx, na, hs, {g0}, Rows{{v1}, {v1}}, {s1, s2}, 2).err.status == PZ_ERR_INVALID, "pballot refuses s_i of different widths");
    CHECK(pc.pballot(ctx, na, hs, {g0}, Rows{{v1}}, {s5}, 2).err.status == PZ_ERR_INVALID, "pballot refuses an s wider than n^2");
    CHECK(pc.pballot(ctx, na, na, {g0}, Rows{{v1}}, {s1}, 2).err.status == PZ_ERR_INVALID, "pballot refuses an hs assigned at n's width");
    CHECK(pc.pballot(ctx, na, hs, {g0, na}, Rows{{v1, v1}}, {s1}, 2).err.status == PZ_ERR_INVALID, "pballot refuses a base assigned at n's width");
    auto big = chip.assign_integer(ctx, n * n, 256).unwrap();
    CHECK(pc.pballot(ctx, na, big, {g0}, Rows{{v1}}, {s1}, 2).err.status == PZ_ERR_RANGE, "pballot refuses hs = n^2 (PZ_ERR_RANGE)");
    CHECK(pc.pballot(ctx, na, hs, {g0, big}, Rows{{v1, v1}}, {s1}, 2).err.status == PZ_ERR_RANGE, "pballot refuses a base of n^2 (PZ_ERR_RANGE)");
    CHECK(!pballot_bases(ctx, n, n + BigUint(1), 16, 8).ok && !pballot_bases(ctx, n, n + BigUint(1), 0, 8).ok &&
              !pballot_bases(ctx, BigUint(14), BigUint(3), 1, 1).ok,
          "pballot_bases refuses 2^(K w) > n, no slot and an even modulus");
}

// what needs no device: the cell counts' refusals over the C ABI, the statement's size, the unpacking
static void test_host_only() {
    size_t a = 0, l = 0;
    CHECK(pz_pballot_cells(2, 64, 10, 2, 3, 1, 1, &a, &l) == PZ_OK && a > 0 && l > 0, "pz_pballot_cells counts a shape");
    size_t a1 = 0, l1 = 0, as = 0, ls = 0;
    // one ciphertext of one slot against the short-randomness ballot of one ciphertext: the same blocks; the base stands at full width
    // where g stood at n's
    size_t narrow = 0, wide = 0;
    CHECK(pz_pballot_cells(2, 64, 10, 1, 1, 2, 1, &a1, &l1) == PZ_OK && pz_sballot_cells(2, 64, 10, 1, 2, 1, &as, &ls) == PZ_OK &&
              pz_op_cells(0, 2, 64, 10, &narrow, nullptr) == PZ_OK && pz_op_cells(0, 4, 64, 10, &wide, nullptr) == PZ_OK &&
              a1 == as - narrow + wide,
          "K = 1: kind 9's cells with g assigned at full width");
    CHECK(pz_pballot_cells(2, 64, 10, 0, 1, 1, 1, &a, &l) == PZ_ERR_INVALID && pz_pballot_cells(2, 64, 10, 2, 0, 1, 1, &a, &l) == PZ_ERR_INVALID &&
              pz_pballot_cells(2, 64, 10, 2, 65, 1, 1, &a, &l) == PZ_ERR_INVALID && pz_pballot_cells(2, 64, 10, 513, 2, 1, 1, &a, &l) == PZ_ERR_INVALID &&
              pz_pballot_cells(2, 64, 10, 2, 2, 65, 1, &a, &l) == PZ_ERR_INVALID && pz_pballot_cells(2, 64, 10, 2, 2, 1, 0, &a, &l) == PZ_ERR_INVALID &&
              pz_pballot_cells(2, 64, 10, 2, 2, 1, 5, &a, &l) == PZ_ERR_INVALID,
          "pz_pballot_cells refuses a shape out of range");
    size_t npub = 0;
    CHECK(pz_pballot_public_cells(2, 64, 10, 2, 3, 2, 2, nullptr, 0, &npub) == PZ_OK && npub == 2 + 4 * (1 + 3 + 2) + 2,
          "pz_pballot_public_cells counts the statement");
    CHECK(pz_pballot_public_cells(2, 64, 10, 2, 1, 2, 2, nullptr, 0, &npub) == PZ_OK && npub == 2 + 4 * (1 + 1 + 2), "... without sums for one slot");
    const std::vector<BigUint> c = unpack_tally(BigUint(0x030201), 3, 8).unwrap();
    CHECK(c.size() == 3 && c[0] == BigUint(1) && c[1] == BigUint(2) && c[2] == BigUint(3) && !unpack_tally(BigUint(0x01000000), 3, 8).ok,
          "unpack_tally: the counts slot by slot");
}

int main(int argc, char** argv) {
    try {
        test_host_only();
        if (argc > 1 && std::strcmp(argv[1], "--host-only") == 0) {
            if (failures) std::printf("%d FAILURES\n", failures);
            else std::printf("ALL OK\n");
            return failures ? 1 : 0;
        }
        test_pballot(128, 64, 13, 2, 3, 2, 8, 2);      // PB1
        test_pballot(128, 64, 10, 1, 1, 1, 8, 1);      // PB3
        test_pballot(264, 88, 11, 1, 2, 1, 16, 1);     // PB2
        test_refusals();
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (failures) {
        std::printf("%d FAILURES\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
