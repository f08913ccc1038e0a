// The tally's host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierChip::tally, paillier_tally_test,
// synthesize_tally_circuit) on seeded inputs: the tape's operation order is the circuit's, its cell totals
// are pz_circuit_cells(3, ..), the root is the product by the C oracle's mul_mod in the product tree's order, and the device
// expansion of the tape ends in assert_equal_fresh's bit -- 1 for the honest product, 0 for a wrong one.
#include <cstdio>
#include <cstring>
#include <random>

#include <hip/hip_runtime_api.h>

#include "../../paillier_halo2_amd/host/paillier_chip.hpp"

extern "C" int ora_mul_mod_step(uint32_t L, const uint64_t* a, const uint64_t* b, const uint64_t* mod, uint64_t* q, uint64_t* r);

using namespace pz;

static std::mt19937_64 rng(0x7a50);
static BigUint gen_biguint(unsigned bits) {
    std::vector<uint64_t> v((bits + 63) / 64);
    for (auto& w : v) w = rng();
    if (bits % 64) v.back() &= (1ull << (bits % 64)) - 1;
    return BigUint::from_limbs(v.data(), v.size());
}
static BigUint oracle_mul(const BigUint& n2, const BigUint& a, const BigUint& b, unsigned L) {
    auto nv = n2.to_limbs(L), av = a.to_limbs(L), bv = b.to_limbs(L);
    std::vector<uint64_t> q(L), r(L);
    if (ora_mul_mod_step(L, av.data(), bv.data(), nv.data(), q.data(), r.data()) != 0) throw std::runtime_error("oracle");
    return BigUint::from_limbs(r.data(), L);
}
// the product tree, restated: neighbours of the current list, an odd last element carried up
static BigUint oracle_tally(const BigUint& n, std::vector<BigUint> cur, unsigned L) {
    const BigUint n2 = n * n;
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

static void test_tally(unsigned enc_bits, unsigned limb_bits, unsigned lookup_bits, unsigned B) {
    static const uint64_t ONE[4] = {0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL};
    Context ctx(0);
    RangeChip range{lookup_bits};
    BigUint n = gen_biguint(enc_bits);
    n = n + (BigUint(1) << (enc_bits - 1));          // a full-size modulus: every ciphertext below 2^(2 enc_bits - 2) is below n^2
    n = n.low_bits(enc_bits);
    if (n.bits() < enc_bits) n = n + (BigUint(1) << (enc_bits - 1));
    std::vector<BigUint> cts;
    for (unsigned i = 0; i < B; ++i) cts.push_back(gen_biguint(2 * enc_bits - 2));
    const unsigned L64 = (2 * enc_bits + 63) / 64;
    BigUint res = oracle_tally(n, cts, L64);
    paillier_tally_test(ctx, range, PaillierTallyInput{limb_bits, enc_bits, n, cts, res});   // throws on any mismatch
    char name[160];
    std::snprintf(name, sizeof name, "paillier_tally_test enc_bits=%u limb_bits=%u B=%u: %zu mul_mod steps, %u limbs in %u words", enc_bits,
                  limb_bits, B, ctx.n_steps(), ctx.limbs(), ctx.words());
    CHECK(ctx.n_steps() == B - 1 && ctx.limbs() == 2 * enc_bits / limb_bits && ctx.words() == L64, name);
    // operation order: assign n, B assigns, square, refresh, the B - 1 steps, assign res, assert -- no load_zero, no constants
    std::vector<int> want(1 + B, 0), got;
    want.insert(want.end(), {1, 2, 4, 0, 5});
    for (auto& o : ctx.ops()) got.push_back((int)o.op);
    CHECK(got == want && ctx.ops()[B + 3].count == B - 1, "operation order of the tape (DESIGN.md section 15.7)");
    const unsigned Ln = enc_bits / limb_bits;
    size_t a = 0, l = 0;
    int rc = pz_circuit_cells(3, Ln, limb_bits, lookup_bits, B - 1, 0, &a, &l);
    CHECK(rc == PZ_OK && a == ctx.advice_cells() && l == ctx.lookup_cells(), "tape cell totals == pz_circuit_cells(3, ..)");
    // the tape's last record holds the root; its first is (c_1, c_2)
    const std::vector<uint64_t>& tp = ctx.tape();
    CHECK(BigUint::from_limbs(tp.data(), L64) == cts[0] && BigUint::from_limbs(tp.data() + L64, L64) == cts[1] &&
              BigUint::from_limbs(tp.data() + ((size_t)(B - 2) * 4 + 3) * L64, L64) == res,
          "records: the first is (c_1, c_2), the last one's remainder is the root");
    uint64_t *d_steps = nullptr, *d_mod = nullptr, *d_adv = nullptr, *d_lk = nullptr;
    std::vector<uint64_t> mod = ctx.modulus().to_limbs(ctx.words());
    bool ok = hipMalloc((void**)&d_steps, tp.size() * 8) == hipSuccess && hipMalloc((void**)&d_mod, mod.size() * 8) == hipSuccess &&
              hipMalloc((void**)&d_adv, a * 32) == hipSuccess && hipMalloc((void**)&d_lk, l * 32 + 32) == hipSuccess;
    ok = ok && hipMemcpy(d_steps, tp.data(), tp.size() * 8, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_mod, mod.data(), mod.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
    uint64_t last[4] = {0, 0, 0, 0}, last_bad[4] = {1, 1, 1, 1};
    if (ok) {
        ok = synthesize_tally_circuit(ctx, enc_bits, n, cts, res, d_steps, d_mod, d_adv, d_lk) == PZ_OK && pz_sync(ctx.raw()) == PZ_OK &&
             hipMemcpy(last, d_adv + 4 * (a - 1), 32, hipMemcpyDeviceToHost) == hipSuccess;
        BigUint wrong = res + BigUint(1);
        ok = ok && synthesize_tally_circuit(ctx, enc_bits, n, cts, wrong, d_steps, d_mod, d_adv, d_lk) == PZ_OK && pz_sync(ctx.raw()) == PZ_OK &&
             hipMemcpy(last_bad, d_adv + 4 * (a - 1), 32, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d_steps); (void)hipFree(d_mod); (void)hipFree(d_adv); (void)hipFree(d_lk);
    CHECK(ok && std::memcmp(last, ONE, 32) == 0, "device expansion of the tally's tape ends in assert_equal_fresh == 1");
    CHECK(ok && (last_bad[0] | last_bad[1] | last_bad[2] | last_bad[3]) == 0, "a wrong `res` expands to assert_equal_fresh == 0");
}

static void test_refusals() {
    Context ctx(0);
    RangeChip range{10};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
    BigUint n = gen_biguint(128) + (BigUint(1) << 127);
    n = n.low_bits(128);
    if (n.bits() < 128) n = n + (BigUint(1) << 127);
    auto na = chip.assign_integer(ctx, n, 128).unwrap();
    EncryptionPublicKeyAssigned pk{na, {}};
    auto c = chip.assign_integer(ctx, gen_biguint(250), 256).unwrap();
    auto narrow = chip.assign_integer(ctx, gen_biguint(120), 128).unwrap();
    CHECK(pc.tally(ctx, pk, {c}).err.status == PZ_ERR_INVALID, "tally refuses a single ciphertext");
    CHECK(pc.tally(ctx, pk, {c, narrow}).err.status == PZ_ERR_INVALID, "tally refuses a ciphertext assigned at enc_bits");
    auto big = chip.assign_integer(ctx, n * n, 256).unwrap();
    CHECK(pc.tally(ctx, pk, {c, big}).err.status == PZ_ERR_RANGE, "tally refuses a ciphertext equal to n^2 (PZ_ERR_RANGE)");
}

int main() {
    try {
        test_tally(128, 64, 10, 5);
        test_tally(128, 64, 10, 8);
        test_tally(264, 88, 11, 3);
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
