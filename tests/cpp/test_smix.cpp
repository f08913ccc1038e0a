// The short-randomness mix's host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierChip::smix, paillier_smix_test,
// synthesize_smix_circuit) on seeded inputs, over the C ABI alone and self-checking with host/biguint.hpp: the
// tape's operation order is the circuit's, its cell totals are pz_smix_cells, every output is c_perm(i) hs^s_i mod n^2 by BigUint
// arithmetic, the route layers are benes_apply's, the records are pz_paillier_smix's, the device expansion of the tape holds the
// statement n | hs | c_1 .. c_K | c'_1 .. c'_K at pz_smix_public_cells and every assert_equal_fresh's bit -- 1 for the honest results,
// 0 for a wrong one.  `--host-only` stops before anything needs a device.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>

#include <hip/hip_runtime_api.h>

#include "../../paillier_halo2_amd/host/paillier_chip.hpp"

using namespace pz;

static std::mt19937_64 rng(0x5d50);
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

static void test_smix(unsigned enc_bits, unsigned limb_bits, unsigned lookup_bits, unsigned K, unsigned s_limbs) {
    static const uint64_t ONE[4] = {0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL};
    Context ctx(0);
    RangeChip range{lookup_bits};
    const BigUint n = gen_modulus(enc_bits), n2 = n * n;
    const unsigned L64 = (2 * enc_bits + 63) / 64, wn = (enc_bits + 63) / 64, wk = 2 * wn, Ln = enc_bits / limb_bits;
    const unsigned s_bits = s_limbs * limb_bits, sw = (s_bits + 63) / 64;
    const std::vector<uint64_t> nw = n.to_limbs(wn);
    // hs as the key authority makes it: (-x^2 mod n)^n mod n^2 (any unit serves the arithmetic checked here)
    BigUint x;
    do x = gen_biguint(enc_bits - 1);
    while (x < BigUint(2) || BigUint::gcd(x, n) != BigUint(1));
    const BigUint hs = pow_mod((n - (x * x) % n) % n, n, n2);
    std::vector<uint32_t> perm(K);
    std::iota(perm.begin(), perm.end(), 0u);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<BigUint> cts, ss, res;
    const BigUint s_all = (BigUint(1) << s_bits) - BigUint(1);
    for (unsigned i = 0; i < K; ++i) {
        cts.push_back(i == 1 ? n2 - BigUint(1) : gen_biguint(2 * enc_bits) % n2);     // (the largest value below n^2 among them)
        ss.push_back(i == 1 ? BigUint(1) << (s_bits - 1) : i == 2 ? s_all : i == 3 ? BigUint(0) : gen_biguint(s_bits));   // a lone top bit, all ones, 0
    }
    for (unsigned i = 0; i < K; ++i) res.push_back(cts[perm[i]] * pow_mod(hs, ss[i], n2) % n2);
    PaillierChip::MixWitness wit;
    paillier_smix_test(ctx, range, PaillierSMixInput{limb_bits, enc_bits, s_limbs, n, hs, cts, perm, ss, res}, &wit);   // throws on any mismatch
    const size_t per = 2 * (size_t)s_bits + 1, ns = K * per, layers = benes_layers(K), n_switch = layers * (K / 2);
    char name[220];
    std::snprintf(name, sizeof name, "paillier_smix_test enc_bits=%u limb_bits=%u K=%u s_limbs=%u: %zu mul_mod steps, %zu switches, %u limbs in %u words",
                  enc_bits, limb_bits, K, s_limbs, ctx.n_steps(), n_switch, ctx.limbs(), ctx.words());
    CHECK(ctx.n_steps() == ns && ctx.limbs() == 2 * Ln && ctx.words() == L64, name);
    // operation order: assign n, hs, K assigns at full width, K assigns of s, square, refresh, load_zero, the switches, per output [const,
    // const, per limb of s (num_to_bits, W x (mul_mod, select)) with a mul_mod between the limbs, mul_mod (the last square and the final
    // block: one record of 2)], then per output assign res, assert.  The tape merges neighbouring mul_mod records.
    std::vector<int> want(2 + 2 * K, Context::ASSIGN), got;
    want.insert(want.end(), {Context::SQUARE, Context::REFRESH, Context::CONST_CELL});
    want.insert(want.end(), n_switch, Context::SWITCH);
    for (unsigned i = 0; i < K; ++i) {
        want.insert(want.end(), {Context::CONST_CELL, Context::CONST_CELL});
        for (unsigned li = 0; li < s_limbs; ++li) {
            want.push_back(Context::NUM_TO_BITS);
            for (unsigned j = 0; j < limb_bits; ++j) want.insert(want.end(), {Context::MUL_MOD, Context::SELECT});
            want.push_back(Context::MUL_MOD);
        }
    }
    for (unsigned i = 0; i < K; ++i) want.insert(want.end(), {Context::ASSIGN, Context::ASSERT_EQUAL});
    for (auto& o : ctx.ops()) got.push_back((int)o.op);
    CHECK(got == want && ctx.ops()[got.size() - 2 * K - 1].count == 2, "operation order of the tape (DESIGN.md section 15.20)");
    size_t a = 0, l = 0;
    int rc = pz_smix_cells(Ln, limb_bits, lookup_bits, K, s_limbs, &a, &l);
    CHECK(rc == PZ_OK && a == ctx.advice_cells() && l == ctx.lookup_cells(), "tape cell totals == pz_smix_cells");
    // the witness: the bits are benes_route's, the route layers benes_apply's over the ciphertexts, the last layer is perm's order
    {
        std::vector<uint8_t> bits;
        bool same = benes_route(K, perm.data(), bits) && bits == wit.bits && wit.routes.size() == layers * K * wk;
        const auto lay = benes_apply(K, bits, cts);
        for (size_t ly = 0; same && ly < layers; ++ly)
            for (size_t j = 0; same && j < K; ++j) same = BigUint::from_limbs(wit.routes.data() + (ly * K + j) * wk, wk) == lay[ly][j];
        for (size_t i = 0; same && layers && i < K; ++i) same = lay.back()[i] == cts[perm[i]];
        CHECK(same, "the witness holds benes_route's bits and benes_apply's layers; the last layer is the permuted list");
    }
    // records: the tape is pz_paillier_smix's records (repacked to the tape's width), output-major
    const std::vector<uint64_t>& tp = ctx.tape();
    {
        std::vector<uint64_t> hw = hs.to_limbs(wk), cv, sv, rec(ns * 4 * wk), mv(K * wk);
        for (const BigUint& c : cts) {
            std::vector<uint64_t> w = c.to_limbs(wk);
            cv.insert(cv.end(), w.begin(), w.end());
        }
        for (const BigUint& s : ss) {
            std::vector<uint64_t> w = s.to_limbs(sw);
            sv.insert(sv.end(), w.begin(), w.end());
        }
        rc = pz_paillier_smix(ctx.raw(), wn, K, s_bits, nw.data(), hw.data(), cv.data(), wit.bits.empty() ? nullptr : wit.bits.data(), sv.data(), nullptr,
                              rec.data(), ns, mv.data());
        bool same = rc == PZ_OK && tp.size() == ns * 4 * L64;
        for (size_t f = 0; same && f < ns * 4; ++f) same = std::memcmp(tp.data() + f * L64, rec.data() + f * wk, L64 * 8) == 0;
        for (unsigned i = 0; same && i < K; ++i) same = BigUint::from_limbs(mv.data() + i * wk, wk) == res[i];
        CHECK(same, "records == pz_paillier_smix's, outputs == c_perm(i) hs^s_i mod n^2 in BigUint arithmetic");
    }
    bool recs = tp.size() == ns * 4 * L64;
    for (unsigned i = 0; recs && i < K; ++i) {
        const uint64_t *first = tp.data() + (size_t)i * per * 4 * L64, *fin = tp.data() + ((size_t)(i + 1) * per - 1) * 4 * L64;
        recs = BigUint::from_limbs(first, L64) == BigUint(1) && BigUint::from_limbs(first + L64, L64) == hs &&
               BigUint::from_limbs(fin, L64) == cts[perm[i]] && BigUint::from_limbs(fin + L64, L64) == pow_mod(hs, ss[i], n2) &&
               BigUint::from_limbs(fin + 3 * L64, L64) == res[i];
    }
    CHECK(recs, "records: every output's chain starts from (1, hs), its last record is (c_perm(i), hs^s_i, q, c'_i)");
    uint64_t *d_work = nullptr, *d_mod = nullptr, *d_adv = nullptr, *d_lk = nullptr;
    std::vector<uint64_t> mod = ctx.modulus().to_limbs(ctx.words());
    bool ok = hipMalloc((void**)&d_work, (ns * 4 + layers * K) * wk * 8 + 64) == hipSuccess && hipMalloc((void**)&d_mod, mod.size() * 8) == hipSuccess &&
              hipMalloc((void**)&d_adv, a * 32) == hipSuccess && hipMalloc((void**)&d_lk, l * 32 + 32) == hipSuccess;
    ok = ok && hipMemcpy(d_mod, mod.data(), mod.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
    size_t a_res = 0, a_eq = 0;
    ok = ok && pz_op_cells(0, 2 * Ln, limb_bits, lookup_bits, &a_res, nullptr) == PZ_OK && pz_op_cells(5, 2 * Ln, limb_bits, lookup_bits, &a_eq, nullptr) == PZ_OK;
    bool bits_one = ok, statement = ok, wrong_zero = ok;
    if (ok) {
        ok = synthesize_smix_circuit(ctx, enc_bits, s_limbs, n, hs, cts, ss, res, wit, d_work, d_mod, d_adv, d_lk) == PZ_OK && pz_sync(ctx.raw()) == PZ_OK;
        for (unsigned i = 0; ok && i < K; ++i) {   // output i's assert_equal_fresh ends (K - 1 - i) result blocks before the stream's end
            uint64_t last[4];
            ok = hipMemcpy(last, d_adv + 4 * (a - 1 - (size_t)(K - 1 - i) * (a_res + a_eq)), 32, hipMemcpyDeviceToHost) == hipSuccess;
            bits_one = bits_one && ok && std::memcmp(last, ONE, 32) == 0;
        }
        // the statement: n | hs | c_1 .. c_K | c'_1 .. c'_K, limb by limb, at the cells pz_smix_public_cells names
        std::vector<uint64_t> cells(Ln + (2 * K + 1) * 2 * Ln);
        size_t npub = 0;
        ok = ok && pz_smix_public_cells(Ln, limb_bits, lookup_bits, K, s_limbs, cells.data(), cells.size(), &npub) == PZ_OK;
        statement = ok && npub == cells.size();
        std::vector<BigUint> want_st;
        auto limbs_of = [&](const BigUint& v, unsigned cnt) {
            for (unsigned j = 0; j < cnt; ++j) want_st.push_back((v >> (j * limb_bits)).low_bits(limb_bits));
        };
        limbs_of(n, Ln);
        limbs_of(hs, 2 * Ln);
        for (const BigUint& c : cts) limbs_of(c, 2 * Ln);
        for (const BigUint& c : res) limbs_of(c, 2 * Ln);
        for (size_t i = 0; statement && i < npub; ++i) statement = cell_is(ctx, d_adv, cells[i], want_st[i]);
        std::vector<BigUint> wrong = res;
        wrong.back() = wrong.back() + BigUint(1);
        uint64_t last_bad[4] = {1, 1, 1, 1}, first_ok[4] = {0, 0, 0, 0};
        wrong_zero = ok && synthesize_smix_circuit(ctx, enc_bits, s_limbs, n, hs, cts, ss, wrong, wit, d_work, d_mod, d_adv, d_lk) == PZ_OK &&
                     pz_sync(ctx.raw()) == PZ_OK && hipMemcpy(last_bad, d_adv + 4 * (a - 1), 32, hipMemcpyDeviceToHost) == hipSuccess &&
                     hipMemcpy(first_ok, d_adv + 4 * (a - 1 - (size_t)(K - 1) * (a_res + a_eq)), 32, hipMemcpyDeviceToHost) == hipSuccess;
        wrong_zero = wrong_zero && (last_bad[0] | last_bad[1] | last_bad[2] | last_bad[3]) == 0 && (K == 1 || std::memcmp(first_ok, ONE, 32) == 0);
    }
    wit.wipe();
    (void)hipFree(d_work); (void)hipFree(d_mod); (void)hipFree(d_adv); (void)hipFree(d_lk);
    CHECK(ok && bits_one, "device expansion of the tape: every assert_equal_fresh == 1");
    CHECK(ok && statement, "the exposed cells hold n | hs | c_1 .. c_K | c'_1 .. c'_K");
    CHECK(ok && wrong_zero, "a wrong last `res` expands to assert_equal_fresh == 0 for that output alone");
}

static void test_refusals() {
    Context ctx(0);
    RangeChip range{10};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
    const BigUint n = gen_modulus(128);
    auto na = chip.assign_integer(ctx, n, 128).unwrap();
    auto hs = chip.assign_integer(ctx, gen_biguint(250), 256).unwrap();
    auto c = chip.assign_integer(ctx, gen_biguint(250), 256).unwrap();
    auto over = chip.assign_integer(ctx, n * n, 256).unwrap();
    auto s1 = chip.assign_integer(ctx, gen_biguint(60), 64).unwrap();
    auto s2 = chip.assign_integer(ctx, gen_biguint(120), 128).unwrap();
    auto s5 = chip.assign_integer(ctx, gen_biguint(300), 320).unwrap();
    CHECK(pc.smix(ctx, na, hs, {c, c, c}, {0, 1, 2}, {s1, s1, s1}, nullptr).err.status == PZ_ERR_INVALID, "smix refuses three ciphertexts");
    CHECK(pc.smix(ctx, na, hs, {c, c}, {0, 1}, {s1}, nullptr).err.status == PZ_ERR_INVALID, "smix refuses a missing s");
    CHECK(pc.smix(ctx, na, hs, {c, c}, {0, 0}, {s1, s1}, nullptr).err.status == PZ_ERR_INVALID, "smix refuses a repeated index");
    CHECK(pc.smix(ctx, na, hs, {c, c}, {0, 2}, {s1, s1}, nullptr).err.status == PZ_ERR_INVALID, "smix refuses an index >= K");
    CHECK(pc.smix(ctx, na, hs, {c, na}, {0, 1}, {s1, s1}, nullptr).err.status == PZ_ERR_INVALID, "smix refuses a ciphertext assigned at n's width");
    CHECK(pc.smix(ctx, na, hs, {c, c}, {0, 1}, {s1, s2}, nullptr).err.status == PZ_ERR_INVALID, "smix refuses s_i of different widths");
    CHECK(pc.smix(ctx, na, hs, {c}, {0}, {s5}, nullptr).err.status == PZ_ERR_INVALID, "smix refuses an s wider than n^2");
    CHECK(pc.smix(ctx, na, na, {c}, {0}, {s1}, nullptr).err.status == PZ_ERR_INVALID, "smix refuses an hs assigned at n's width");
    CHECK(pc.smix(ctx, na, over, {c}, {0}, {s1}, nullptr).err.status == PZ_ERR_RANGE, "smix refuses hs = n^2 (PZ_ERR_RANGE)");
    CHECK(pc.smix(ctx, na, hs, {c, over}, {1, 0}, {s1, s1}, nullptr).err.status == PZ_ERR_RANGE, "smix refuses a ciphertext of n^2 (PZ_ERR_RANGE)");
}

// what needs no device: the cell counts' refusals over the C ABI
static void test_host_only() {
    size_t a = 0, l = 0;
    CHECK(pz_smix_cells(2, 64, 10, 2, 1, &a, &l) == PZ_OK && a > 0 && l > 0, "pz_smix_cells counts a shape");
    CHECK(pz_smix_cells(2, 64, 10, 0, 1, &a, &l) == PZ_ERR_INVALID && pz_smix_cells(2, 64, 10, 3, 1, &a, &l) == PZ_ERR_INVALID &&
              pz_smix_cells(2, 64, 10, 2048, 1, &a, &l) == PZ_ERR_INVALID && pz_smix_cells(2, 64, 10, 2, 0, &a, &l) == PZ_ERR_INVALID &&
              pz_smix_cells(2, 64, 10, 2, 5, &a, &l) == PZ_ERR_INVALID,
          "pz_smix_cells refuses a shape out of range");
    size_t npub = 0;
    CHECK(pz_smix_public_cells(2, 64, 10, 4, 2, nullptr, 0, &npub) == PZ_OK && npub == 2 + 4 + 2 * 4 * 4, "pz_smix_public_cells counts the statement");
}

int main(int argc, char** argv) {
    try {
        test_host_only();
        if (!(argc > 1 && std::strcmp(argv[1], "--host-only") == 0)) {
            test_smix(128, 64, 13, 4, 2);      // SX4
            test_smix(128, 64, 10, 1, 1);
            test_smix(264, 88, 11, 2, 1);
            test_refusals();
        }
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
