// The ballot's host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierChip::ballot, paillier_ballot_test,
// synthesize_ballot_circuit) on seeded inputs: the tape's operation order is the circuit's, its cell totals are
// pz_ballot_cells, its records are pz_paillier_ballot's, every ciphertext is g^m r^n by the C oracle's mul_mod in the two schedules, the
// device expansion of the tape holds the statement n | g | c_1 .. c_K | S at pz_ballot_public_cells and every assert_equal_fresh's bit --
// 1 for the honest results, 0 for a wrong one.
#include <cstdio>
#include <cstring>
#include <random>

#include <hip/hip_runtime_api.h>

#include "../../paillier_halo2_amd/host/paillier_chip.hpp"

extern "C" int ora_mul_mod_step(uint32_t L, const uint64_t* a, const uint64_t* b, const uint64_t* mod, uint64_t* q, uint64_t* r);

using namespace pz;

static std::mt19937_64 rng(0x6b50);
static BigUint gen_biguint(unsigned bits) {
    std::vector<uint64_t> v((bits + 63) / 64);
    for (auto& w : v) w = rng();
    if (bits % 64) v.back() &= (1ull << (bits % 64)) - 1;
    return BigUint::from_limbs(v.data(), v.size());
}
static BigUint gen_modulus(unsigned enc_bits) {   // a full-size modulus
    BigUint n = gen_biguint(enc_bits) + (BigUint(1) << (enc_bits - 1));
    n = n.low_bits(enc_bits);
    if (n.bits() < enc_bits) n = n + (BigUint(1) << (enc_bits - 1));
    return n;
}
static BigUint oracle_mul(const BigUint& n2, const BigUint& a, const BigUint& b, unsigned L) {
    auto nv = n2.to_limbs(L), av = a.to_limbs(L), bv = b.to_limbs(L);
    std::vector<uint64_t> q(L), r(L);
    if (ora_mul_mod_step(L, av.data(), bv.data(), nv.data(), q.data(), r.data()) != 0) throw std::runtime_error("oracle");
    return BigUint::from_limbs(r.data(), L);
}
// square-and-multiply, LSB first, over the exponent's words
static BigUint oracle_pow(const BigUint& n2, const BigUint& base, const std::vector<uint64_t>& e, size_t bits, unsigned L) {
    BigUint acc(1), sq = base;
    for (size_t j = 0; j < bits; ++j) {
        if ((e[j / 64] >> (j % 64)) & 1) acc = oracle_mul(n2, acc, sq, L);
        sq = oracle_mul(n2, sq, sq, L);
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

static void test_ballot(unsigned enc_bits, unsigned limb_bits, unsigned lookup_bits, unsigned K, unsigned m_bits) {
    static const uint64_t ONE[4] = {0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL};
    Context ctx(0);
    RangeChip range{lookup_bits};
    const BigUint n = gen_modulus(enc_bits), n2 = n * n, g = n + BigUint(1);
    const uint64_t mmax = m_bits == 64 ? ~0ull : (1ull << m_bits) - 1;
    const unsigned L64 = (2 * enc_bits + 63) / 64, wn = (enc_bits + 63) / 64;
    const std::vector<uint64_t> nw = n.to_limbs(wn);
    size_t nr = n.bits();
    for (uint64_t w : nw) nr += (size_t)__builtin_popcountll(w);
    std::vector<uint64_t> ms;
    std::vector<BigUint> rs, res;
    BigUint total(0);
    for (unsigned i = 0; i < K; ++i) {
        ms.push_back(i == 0 ? mmax : i == 1 ? 0 : i == 2 ? 1ull << (m_bits - 1) : rng() & mmax);   // all ones, zero, a lone top bit
        rs.push_back(i == 0 ? BigUint(1) : gen_biguint(enc_bits - 1));
        const BigUint gm = oracle_pow(n2, g, std::vector<uint64_t>{ms[i]}, m_bits, L64);
        res.push_back(oracle_mul(n2, gm, oracle_pow(n2, rs[i], nw, n.bits(), L64), L64));
        total = total + BigUint(ms[i]);
    }
    paillier_ballot_test(ctx, range, PaillierBallotInput{limb_bits, enc_bits, m_bits, n, g, ms, rs, res});   // throws on any mismatch
    const size_t per = 2 * (size_t)m_bits + nr + 1, ns = K * per;
    char name[200];
    std::snprintf(name, sizeof name, "paillier_ballot_test enc_bits=%u limb_bits=%u K=%u b=%u: %zu mul_mod steps, %u limbs in %u words", enc_bits,
                  limb_bits, K, m_bits, ctx.n_steps(), ctx.limbs(), ctx.words());
    CHECK(ctx.n_steps() == ns && ctx.limbs() == 2 * enc_bits / limb_bits && ctx.words() == L64, name);
    // operation order: assign n, g, K load_witness, the sum (K >= 2), K assigns, square, refresh, load_zero, per entry [const, const,
    // num_to_bits, b x (mul_mod, select), mul_mod, const, const, mul_mod (the r^n chain and the final block: one record of nr + 1)], then
    // per entry assign res, assert.  The tape merges neighbouring mul_mod records: a bit's square_mod and the next bit's mul_mod.
    std::vector<int> want(2, Context::ASSIGN), got;
    want.insert(want.end(), K, Context::LOAD_WITNESS);
    if (K >= 2) want.push_back(Context::SUM);
    want.insert(want.end(), K, Context::ASSIGN);
    want.insert(want.end(), {Context::SQUARE, Context::REFRESH, Context::CONST_CELL});
    for (unsigned i = 0; i < K; ++i) {
        want.insert(want.end(), {Context::CONST_CELL, Context::CONST_CELL, Context::NUM_TO_BITS});
        for (unsigned j = 0; j < m_bits; ++j) want.insert(want.end(), {Context::MUL_MOD, Context::SELECT});
        want.insert(want.end(), {Context::MUL_MOD, Context::CONST_CELL, Context::CONST_CELL, Context::MUL_MOD});
    }
    for (unsigned i = 0; i < K; ++i) want.insert(want.end(), {Context::ASSIGN, Context::ASSERT_EQUAL});
    for (auto& o : ctx.ops()) got.push_back((int)o.op);
    CHECK(got == want && ctx.ops()[got.size() - 2 * K - 1].count == nr + 1, "operation order of the tape (DESIGN.md section 15.10)");
    const unsigned Ln = enc_bits / limb_bits;
    size_t a = 0, l = 0;
    int rc = pz_ballot_cells(Ln, limb_bits, lookup_bits, K, m_bits, nr, &a, &l);
    CHECK(rc == PZ_OK && a == ctx.advice_cells() && l == ctx.lookup_cells(), "tape cell totals == pz_ballot_cells");
    // records: the tape is pz_paillier_ballot's records (repacked to the tape's width), entry-major
    const std::vector<uint64_t>& tp = ctx.tape();
    {
        std::vector<uint64_t> gw = g.to_limbs(wn), rw, rec(ns * 4 * 2 * wn), cv(K * 2 * wn);
        for (const BigUint& r : rs) {
            std::vector<uint64_t> w = r.to_limbs(wn);
            rw.insert(rw.end(), w.begin(), w.end());
        }
        uint32_t nr_lib = 0;
        rc = pz_paillier_ballot(ctx.raw(), wn, K, m_bits, nw.data(), gw.data(), ms.data(), rw.data(), rec.data(), ns, &nr_lib, cv.data());
        bool same = rc == PZ_OK && nr_lib == nr && tp.size() == ns * 4 * L64;
        for (size_t f = 0; same && f < ns * 4; ++f) same = std::memcmp(tp.data() + f * L64, rec.data() + f * 2 * wn, L64 * 8) == 0;
        for (unsigned i = 0; same && i < K; ++i) same = BigUint::from_limbs(cv.data() + i * 2 * wn, 2 * wn) == res[i];
        CHECK(same, "records == pz_paillier_ballot's, ciphertexts == the oracle's g^m r^n mod n^2");
    }
    bool recs = BigUint::from_limbs(tp.data(), L64) == BigUint(1) && BigUint::from_limbs(tp.data() + L64, L64) == g;
    for (unsigned i = 0; i < K; ++i) recs = recs && BigUint::from_limbs(tp.data() + (((size_t)(i + 1) * per - 1) * 4 + 3) * L64, L64) == res[i];
    CHECK(recs, "records: the first is (1, g), every entry's last remainder is its ciphertext");
    uint64_t *d_steps = nullptr, *d_mod = nullptr, *d_adv = nullptr, *d_lk = nullptr;
    std::vector<uint64_t> mod = ctx.modulus().to_limbs(ctx.words());
    bool ok = hipMalloc((void**)&d_steps, tp.size() * 8) == hipSuccess && hipMalloc((void**)&d_mod, mod.size() * 8) == hipSuccess &&
              hipMalloc((void**)&d_adv, a * 32) == hipSuccess && hipMalloc((void**)&d_lk, l * 32 + 32) == hipSuccess;
    ok = ok && hipMemcpy(d_steps, tp.data(), tp.size() * 8, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_mod, mod.data(), mod.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
    size_t a_res = 0, a_eq = 0;
    ok = ok && pz_op_cells(0, 2 * Ln, limb_bits, lookup_bits, &a_res, nullptr) == PZ_OK && pz_op_cells(5, 2 * Ln, limb_bits, lookup_bits, &a_eq, nullptr) == PZ_OK;
    bool bits_one = ok, statement = ok, wrong_zero = ok;
    if (ok) {
        ok = synthesize_ballot_circuit(ctx, enc_bits, m_bits, nr, n, g, ms, rs, res, d_steps, d_mod, d_adv, d_lk) == PZ_OK && pz_sync(ctx.raw()) == PZ_OK;
        for (unsigned i = 0; ok && i < K; ++i) {   // entry i's assert_equal_fresh ends (K - 1 - i) result blocks before the stream's end
            uint64_t last[4];
            ok = hipMemcpy(last, d_adv + 4 * (a - 1 - (size_t)(K - 1 - i) * (a_res + a_eq)), 32, hipMemcpyDeviceToHost) == hipSuccess;
            bits_one = bits_one && ok && std::memcmp(last, ONE, 32) == 0;
        }
        // the statement: n | g | c_1 .. c_K | S, limb by limb, at the cells pz_ballot_public_cells names
        std::vector<uint64_t> cells(2 * Ln * (K + 1) + 1);
        size_t npub = 0;
        ok = ok && pz_ballot_public_cells(Ln, limb_bits, lookup_bits, K, m_bits, nr, cells.data(), cells.size(), &npub) == PZ_OK;
        statement = ok && npub == 2 * Ln + (size_t)K * 2 * Ln + (K >= 2 ? 1 : 0);
        std::vector<BigUint> want_st;
        auto limbs_of = [&](const BigUint& v, unsigned cnt) {
            for (unsigned j = 0; j < cnt; ++j) want_st.push_back((v >> (j * limb_bits)).low_bits(limb_bits));
        };
        limbs_of(n, Ln);
        limbs_of(g, Ln);
        for (const BigUint& c : res) limbs_of(c, 2 * Ln);
        if (K >= 2) want_st.push_back(total);
        for (size_t i = 0; statement && i < npub; ++i) statement = cell_is(ctx, d_adv, cells[i], want_st[i]);
        std::vector<BigUint> wrong = res;
        wrong.back() = wrong.back() + BigUint(1);
        uint64_t last_bad[4] = {1, 1, 1, 1}, first_ok[4] = {0, 0, 0, 0};
        wrong_zero = ok && synthesize_ballot_circuit(ctx, enc_bits, m_bits, nr, n, g, ms, rs, wrong, d_steps, d_mod, d_adv, d_lk) == PZ_OK &&
                     pz_sync(ctx.raw()) == PZ_OK && hipMemcpy(last_bad, d_adv + 4 * (a - 1), 32, hipMemcpyDeviceToHost) == hipSuccess &&
                     hipMemcpy(first_ok, d_adv + 4 * (a - 1 - (size_t)(K - 1) * (a_res + a_eq)), 32, hipMemcpyDeviceToHost) == hipSuccess;
        wrong_zero = wrong_zero && (last_bad[0] | last_bad[1] | last_bad[2] | last_bad[3]) == 0 && (K == 1 || std::memcmp(first_ok, ONE, 32) == 0);
    }
    (void)hipFree(d_steps); (void)hipFree(d_mod); (void)hipFree(d_adv); (void)hipFree(d_lk);
    CHECK(ok && bits_one, "device expansion of the ballot's tape: every assert_equal_fresh == 1");
    CHECK(ok && statement, "the exposed cells hold n | g | c_1 .. c_K | S");
    CHECK(ok && wrong_zero, "a wrong last `res` expands to assert_equal_fresh == 0 for that entry alone");
}

static void test_refusals() {
    Context ctx(0);
    RangeChip range{10};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
    const BigUint n = gen_modulus(128);
    auto na = chip.assign_integer(ctx, n, 128).unwrap();
    auto ga = chip.assign_integer(ctx, n + BigUint(1), 128).unwrap();
    EncryptionPublicKeyAssigned pk{na, ga};
    auto r = chip.assign_integer(ctx, gen_biguint(120), 128).unwrap();
    auto wide = chip.assign_integer(ctx, gen_biguint(250), 256).unwrap();
    const AssignedWeight m1{1, ctx.load_witness()}, m4{4, ctx.load_witness()};
    CHECK(pc.ballot(ctx, pk, {m4}, {r}, 2).err.status == PZ_ERR_MESSAGE_RANGE, "ballot refuses a message of 2^b (PZ_ERR_MESSAGE_RANGE)");
    CHECK(pc.ballot(ctx, pk, {m1}, {r}, 0).err.status == PZ_ERR_INVALID && pc.ballot(ctx, pk, {m1}, {r}, 65).err.status == PZ_ERR_INVALID,
          "ballot refuses b = 0 and b = 65");
    CHECK(pc.ballot(ctx, pk, {m1, m1}, {r}, 2).err.status == PZ_ERR_INVALID, "ballot refuses a missing r");
    CHECK(pc.ballot(ctx, pk, {}, {}, 2).err.status == PZ_ERR_INVALID, "ballot refuses no message");
    CHECK(pc.ballot(ctx, pk, {m1}, {wide}, 2).err.status == PZ_ERR_INVALID, "ballot refuses an r assigned at full width");
}

int main() {
    try {
        test_ballot(128, 64, 13, 3, 2);      // SB1
        test_ballot(128, 64, 10, 1, 1);
        test_ballot(264, 88, 11, 2, 1);
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
