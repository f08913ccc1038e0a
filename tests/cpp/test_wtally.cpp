// The weighted tally's host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierChip::mul_scalar / weighted_tally,
// paillier_wtally_test, synthesize_wtally_circuit) on seeded inputs: the tape's operation order is the
// circuit's, its cell totals are pz_circuit_cells(4, ..), the root is prod c_i^w_i by the C oracle's mul_mod in pow_mod's schedule and
// the product tree's order, and the device expansion of the tape ends in assert_equal_fresh's bit -- 1 for the honest result, 0 for a
// wrong one.
#include <cstdio>
#include <cstring>
#include <random>

#include <hip/hip_runtime_api.h>

#include "../../paillier_halo2_amd/host/paillier_chip.hpp"

extern "C" int ora_mul_mod_step(uint32_t L, const uint64_t* a, const uint64_t* b, const uint64_t* mod, uint64_t* q, uint64_t* r);

using namespace pz;

static std::mt19937_64 rng(0x3a50);
static BigUint gen_biguint(unsigned bits) {
    std::vector<uint64_t> v((bits + 63) / 64);
    for (auto& w : v) w = rng();
    if (bits % 64) v.back() &= (1ull << (bits % 64)) - 1;
    return BigUint::from_limbs(v.data(), v.size());
}
static BigUint gen_modulus(unsigned enc_bits) {   // a full-size modulus: every ciphertext below 2^(2 enc_bits - 2) is below n^2
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
// pow_mod's uniform schedule, restated: per bit, LSB first, acc takes acc * sq where the bit is set, then sq is squared
static BigUint oracle_pow(const BigUint& n2, const BigUint& c, uint64_t w, unsigned w_bits, unsigned L) {
    BigUint acc(1), sq = c;
    for (unsigned j = 0; j < w_bits; ++j) {
        const BigUint mul = oracle_mul(n2, acc, sq, L);
        if ((w >> j) & 1) acc = mul;
        sq = oracle_mul(n2, sq, sq, L);
    }
    return acc;
}
// the product tree, restated: neighbours of the current list, an odd last element carried up
static BigUint oracle_tree(const BigUint& n2, std::vector<BigUint> cur, unsigned L) {
    while (cur.size() > 1) {
        std::vector<BigUint> nxt;
        for (size_t j = 0; j + 1 < cur.size(); j += 2) nxt.push_back(oracle_mul(n2, cur[j], cur[j + 1], L));
        if (cur.size() & 1) nxt.push_back(cur.back());
        cur.swap(nxt);
    }
    return cur[0];
}

static int failures = 0;
#define CHECK(cond, what)                                          \
    do {                                                           \
        if (!(cond)) { std::printf("FAIL %s\n", what); ++failures; } \
        else std::printf("ok   %s\n", what);                       \
    } while (0)

static void test_wtally(unsigned enc_bits, unsigned limb_bits, unsigned lookup_bits, unsigned B, unsigned w_bits) {
    static const uint64_t ONE[4] = {0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL};
    Context ctx(0);
    RangeChip range{lookup_bits};
    const BigUint n = gen_modulus(enc_bits), n2 = n * n;
    const uint64_t wmax = w_bits == 64 ? ~0ull : (1ull << w_bits) - 1;
    std::vector<BigUint> cts, powers;
    std::vector<uint64_t> weights;
    const unsigned L64 = (2 * enc_bits + 63) / 64;
    for (unsigned i = 0; i < B; ++i) {
        cts.push_back(gen_biguint(2 * enc_bits - 2));
        weights.push_back(i == 0 ? 0 : i == 1 ? wmax : i == 2 ? 1ull << (w_bits - 1) : rng() & wmax);   // zero, all ones, a lone top bit
        powers.push_back(oracle_pow(n2, cts[i], weights[i], w_bits, L64));
    }
    if (B == 1) {   // (one chain: give it the all-ones weight, so that the result is not the constant 1)
        weights[0] = wmax;
        powers[0] = oracle_pow(n2, cts[0], wmax, w_bits, L64);
    }
    const BigUint res = oracle_tree(n2, powers, L64);
    paillier_wtally_test(ctx, range, PaillierWTallyInput{limb_bits, enc_bits, w_bits, n, cts, weights, res});   // throws on any mismatch
    const size_t ng = 2 * (size_t)B * w_bits, ns = ng + B - 1;
    char name[200];
    std::snprintf(name, sizeof name, "paillier_wtally_test enc_bits=%u limb_bits=%u B=%u W=%u: %zu mul_mod steps, %u limbs in %u words", enc_bits,
                  limb_bits, B, w_bits, ctx.n_steps(), ctx.limbs(), ctx.words());
    CHECK(ctx.n_steps() == ns && ctx.limbs() == 2 * enc_bits / limb_bits && ctx.words() == L64, name);
    // operation order: assign n, B assigns, B load_witness, square, refresh, per chain [const, const, num_to_bits, W x (mul_mod, select,
    // square_mod)], the tree's steps, assign res, assert.  The tape merges neighbouring mul_mod records: a bit's square_mod and the next
    // bit's mul_mod are one record of two steps, the last chain's last square_mod and the tree's B - 1 steps one of B.
    std::vector<int> want(1 + B, Context::ASSIGN), got;
    want.insert(want.end(), B, Context::LOAD_WITNESS);
    want.insert(want.end(), {Context::SQUARE, Context::REFRESH});
    for (unsigned i = 0; i < B; ++i) {
        want.insert(want.end(), {Context::CONST_CELL, Context::CONST_CELL, Context::NUM_TO_BITS});
        for (unsigned j = 0; j < w_bits; ++j) want.insert(want.end(), {Context::MUL_MOD, Context::SELECT});
        want.push_back(Context::MUL_MOD);
    }
    want.insert(want.end(), {Context::ASSIGN, Context::ASSERT_EQUAL});
    for (auto& o : ctx.ops()) got.push_back((int)o.op);
    CHECK(got == want && ctx.ops()[got.size() - 3].count == (size_t)B, "operation order of the tape (DESIGN.md section 15.8)");
    const unsigned Ln = enc_bits / limb_bits;
    size_t a = 0, l = 0;
    int rc = pz_circuit_cells(4, Ln, limb_bits, lookup_bits, ng, B - 1, &a, &l);
    CHECK(rc == PZ_OK && a == ctx.advice_cells() && l == ctx.lookup_cells(), "tape cell totals == pz_circuit_cells(4, ..)");
    // the tape's first record is (1, c_1); with a tree, the last one's remainder is the root
    const std::vector<uint64_t>& tp = ctx.tape();
    bool recs = BigUint::from_limbs(tp.data(), L64) == BigUint(1) && BigUint::from_limbs(tp.data() + L64, L64) == cts[0];
    if (B > 1) recs = recs && BigUint::from_limbs(tp.data() + ((ns - 1) * 4 + 3) * L64, L64) == res;
    CHECK(recs, "records: the first is (1, c_1), the last tree record's remainder is the root");
    uint64_t *d_steps = nullptr, *d_mod = nullptr, *d_adv = nullptr, *d_lk = nullptr;
    std::vector<uint64_t> mod = ctx.modulus().to_limbs(ctx.words());
    bool ok = hipMalloc((void**)&d_steps, tp.size() * 8) == hipSuccess && hipMalloc((void**)&d_mod, mod.size() * 8) == hipSuccess &&
              hipMalloc((void**)&d_adv, a * 32) == hipSuccess && hipMalloc((void**)&d_lk, l * 32 + 32) == hipSuccess;
    ok = ok && hipMemcpy(d_steps, tp.data(), tp.size() * 8, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_mod, mod.data(), mod.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
    uint64_t last[4] = {0, 0, 0, 0}, last_bad[4] = {1, 1, 1, 1};
    if (ok) {
        ok = synthesize_wtally_circuit(ctx, enc_bits, w_bits, n, cts, weights, res, d_steps, d_mod, d_adv, d_lk) == PZ_OK &&
             pz_sync(ctx.raw()) == PZ_OK && hipMemcpy(last, d_adv + 4 * (a - 1), 32, hipMemcpyDeviceToHost) == hipSuccess;
        BigUint wrong = res + BigUint(1);
        ok = ok && synthesize_wtally_circuit(ctx, enc_bits, w_bits, n, cts, weights, wrong, d_steps, d_mod, d_adv, d_lk) == PZ_OK &&
             pz_sync(ctx.raw()) == PZ_OK && hipMemcpy(last_bad, d_adv + 4 * (a - 1), 32, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d_steps); (void)hipFree(d_mod); (void)hipFree(d_adv); (void)hipFree(d_lk);
    CHECK(ok && std::memcmp(last, ONE, 32) == 0, "device expansion of the weighted tally's tape ends in assert_equal_fresh == 1");
    CHECK(ok && (last_bad[0] | last_bad[1] | last_bad[2] | last_bad[3]) == 0, "a wrong `res` expands to assert_equal_fresh == 0");
}

static void test_mul_scalar_and_refusals() {
    Context ctx(0);
    RangeChip range{10};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
    const BigUint n = gen_modulus(128), n2 = n * n;
    auto na = chip.assign_integer(ctx, n, 128).unwrap();
    EncryptionPublicKeyAssigned pk{na, {}};
    const BigUint cv = gen_biguint(250);
    auto c = chip.assign_integer(ctx, cv, 256).unwrap();
    auto narrow = chip.assign_integer(ctx, gen_biguint(120), 128).unwrap();
    const AssignedWeight w5{5, ctx.load_witness()}, w8{8, ctx.load_witness()};
    auto p = pc.mul_scalar(ctx, pk, c, w5, 3);
    BigUint c2 = oracle_mul(n2, cv, cv, 4), c4 = oracle_mul(n2, c2, c2, 4);
    CHECK(p.ok && p.val.value() == oracle_mul(n2, c4, cv, 4), "mul_scalar(c, 5) == c^5 mod n^2");
    CHECK(pc.mul_scalar(ctx, pk, c, w8, 3).err.status == PZ_ERR_MESSAGE_RANGE, "mul_scalar refuses a weight of 2^W (PZ_ERR_MESSAGE_RANGE)");
    CHECK(pc.mul_scalar(ctx, pk, c, w5, 0).err.status == PZ_ERR_INVALID && pc.mul_scalar(ctx, pk, c, w5, 65).err.status == PZ_ERR_INVALID,
          "mul_scalar refuses W = 0 and W = 65");
    CHECK(pc.weighted_tally(ctx, pk, {c, c}, {w5}, 3).err.status == PZ_ERR_INVALID, "weighted_tally refuses a missing weight");
    CHECK(pc.weighted_tally(ctx, pk, {}, {}, 3).err.status == PZ_ERR_INVALID, "weighted_tally refuses no ciphertext");
    CHECK(pc.weighted_tally(ctx, pk, {c, narrow}, {w5, w5}, 3).err.status == PZ_ERR_INVALID,
          "weighted_tally refuses a ciphertext assigned at enc_bits");
    auto big = chip.assign_integer(ctx, n2, 256).unwrap();
    CHECK(pc.weighted_tally(ctx, pk, {c, big}, {w5, w5}, 3).err.status == PZ_ERR_RANGE,
          "weighted_tally refuses a ciphertext equal to n^2 (PZ_ERR_RANGE)");
}

int main() {
    try {
        test_wtally(128, 64, 10, 3, 3);
        test_wtally(128, 64, 10, 1, 4);
        test_wtally(128, 64, 10, 4, 1);
        test_wtally(264, 88, 11, 2, 2);
        test_mul_scalar_and_refusals();
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
