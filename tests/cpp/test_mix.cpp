// The mix's host mirror (paillier_halo2_amd/host/benes.hpp: pz::benes_route / benes_apply; paillier_chip.hpp: PaillierChip::mix,
// paillier_mix_test, synthesize_mix_circuit) on seeded inputs, over the C ABI alone and self-checking with
// host/biguint.hpp: every permutation of 2, 4 and 8 positions and seeded ones up to 1024 route to themselves, pz_mix_route gives the same
// bits and the same refusals; the tape's operation order is the circuit's, its cell totals are pz_mix_cells, every output is
// c_perm(i) r_i^n mod n^2 by BigUint arithmetic, the route layers are benes_apply's, the device expansion of the tape holds the statement
// n | c_1 .. c_K | c'_1 .. c'_K at pz_mix_public_cells and every assert_equal_fresh's bit -- 1 for the honest results, 0 for a wrong one.
// `--route-only` stops before anything needs a device.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>

#include <hip/hip_runtime_api.h>

#include "../../paillier_halo2_amd/host/paillier_chip.hpp"

using namespace pz;

static std::mt19937_64 rng(0x31D0);
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

static bool routes_to_itself(const std::vector<uint32_t>& perm) {
    const size_t K = perm.size();
    std::vector<uint8_t> bits, lib(benes_layers(K) * (K / 2) + 1, 9);
    if (!benes_route(K, perm.data(), bits) || bits.size() != benes_layers(K) * (K / 2)) return false;
    std::vector<uint32_t> xs(K);
    std::iota(xs.begin(), xs.end(), 100u);
    const auto layers = benes_apply(K, bits, xs);
    const std::vector<uint32_t>& out = layers.empty() ? xs : layers.back();
    for (size_t i = 0; i < K; ++i)
        if (out[i] != xs[perm[i]]) return false;
    for (uint8_t b : bits)
        if (b > 1) return false;
    // the entry point runs the same routine
    if (pz_mix_route(K, perm.data(), lib.data()) != PZ_OK || lib.back() != 9) return false;
    return std::equal(bits.begin(), bits.end(), lib.begin());
}

static void test_routing() {
    for (unsigned K : {2u, 4u, 8u}) {
        std::vector<uint32_t> p(K);
        std::iota(p.begin(), p.end(), 0u);
        size_t n = 0;
        bool ok = true;
        do {
            ok = ok && routes_to_itself(p);
            ++n;
        } while (std::next_permutation(p.begin(), p.end()));
        char name[100];
        std::snprintf(name, sizeof name, "every permutation of %u positions routes to itself (%zu)", K, n);
        CHECK(ok && n == (K == 2 ? 2u : K == 4 ? 24u : 40320u), name);
    }
    bool ok = routes_to_itself({0});
    for (unsigned K : {16u, 64u, 1024u}) {
        std::vector<uint32_t> p(K);
        std::iota(p.begin(), p.end(), 0u);
        ok = ok && routes_to_itself(p);
        std::reverse(p.begin(), p.end());
        ok = ok && routes_to_itself(p);
        for (int t = 0; t < 10; ++t) {
            std::shuffle(p.begin(), p.end(), rng);
            ok = ok && routes_to_itself(p);
        }
    }
    CHECK(ok, "the identity, the reversal and seeded permutations of 1, 16, 64 and 1024 positions route to themselves");
    std::vector<uint8_t> bits(8, 9), keep;
    const uint32_t twice[4] = {0, 1, 1, 2}, big[4] = {0, 1, 2, 4}, three[3] = {0, 1, 2}, fine[4] = {3, 1, 0, 2};
    bool refused = pz_mix_route(4, twice, bits.data()) == PZ_ERR_INVALID && pz_mix_route(4, big, bits.data()) == PZ_ERR_INVALID &&
                   pz_mix_route(3, three, bits.data()) == PZ_ERR_INVALID && pz_mix_route(0, three, bits.data()) == PZ_ERR_INVALID &&
                   pz_mix_route(2048, three, bits.data()) == PZ_ERR_INVALID && pz_mix_route(4, nullptr, bits.data()) == PZ_ERR_INVALID &&
                   pz_mix_route(4, fine, nullptr) == PZ_ERR_INVALID;
    refused = refused && std::all_of(bits.begin(), bits.end(), [](uint8_t b) { return b == 9; });
    refused = refused && !benes_route(4, twice, keep) && !benes_route(4, big, keep) && !benes_route(3, three, keep) && keep.empty();
    CHECK(refused, "a repeated index, an index >= K, K = 3, K = 0, K = 2048 and null pointers are refused, nothing written");
}

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

static void test_mix(unsigned enc_bits, unsigned limb_bits, unsigned lookup_bits, unsigned K) {
    static const uint64_t ONE[4] = {0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL};
    Context ctx(0);
    RangeChip range{lookup_bits};
    const BigUint n = gen_modulus(enc_bits), n2 = n * n;
    const unsigned L64 = (2 * enc_bits + 63) / 64, wn = (enc_bits + 63) / 64, wk = 2 * wn, Ln = enc_bits / limb_bits;
    const std::vector<uint64_t> nw = n.to_limbs(wn);
    size_t nr = n.bits();
    for (uint64_t w : nw) nr += (size_t)__builtin_popcountll(w);
    std::vector<uint32_t> perm(K);
    std::iota(perm.begin(), perm.end(), 0u);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<BigUint> cts, rs, res;
    for (unsigned i = 0; i < K; ++i) {
        cts.push_back(i == 1 ? n2 - BigUint(1) : gen_biguint(2 * enc_bits) % n2);     // (the largest value below n^2 among them)
        rs.push_back(i == 0 ? BigUint(1) : gen_biguint(enc_bits - 1));
    }
    for (unsigned i = 0; i < K; ++i) res.push_back(cts[perm[i]] * pow_mod(rs[i], n, n2) % n2);
    PaillierChip::MixWitness wit;
    paillier_mix_test(ctx, range, PaillierMixInput{limb_bits, enc_bits, n, cts, perm, rs, res}, &wit);   // throws on any mismatch
    const size_t per = nr + 1, ns = K * per, layers = benes_layers(K), n_switch = layers * (K / 2);
    char name[200];
    std::snprintf(name, sizeof name, "paillier_mix_test enc_bits=%u limb_bits=%u K=%u: %zu mul_mod steps, %zu switches, %u limbs in %u words", enc_bits,
                  limb_bits, K, ctx.n_steps(), n_switch, ctx.limbs(), ctx.words());
    CHECK(ctx.n_steps() == ns && ctx.limbs() == 2 * Ln && ctx.words() == L64, name);
    // operation order: assign n, K assigns at full width, K assigns, square, refresh, load_zero, the switches, per output [const, const,
    // mul_mod (the r^n chain and the final block: one record of nr + 1)], then per output assign res, assert
    std::vector<int> want(1 + 2 * K, Context::ASSIGN), got;
    want.insert(want.end(), {Context::SQUARE, Context::REFRESH, Context::CONST_CELL});
    want.insert(want.end(), n_switch, Context::SWITCH);
    for (unsigned i = 0; i < K; ++i) want.insert(want.end(), {Context::CONST_CELL, Context::CONST_CELL, Context::MUL_MOD});
    for (unsigned i = 0; i < K; ++i) want.insert(want.end(), {Context::ASSIGN, Context::ASSERT_EQUAL});
    for (auto& o : ctx.ops()) got.push_back((int)o.op);
    CHECK(got == want && ctx.ops()[got.size() - 2 * K - 1].count == nr + 1, "operation order of the tape (DESIGN.md section 15.17)");
    size_t a = 0, l = 0;
    int rc = pz_mix_cells(Ln, limb_bits, lookup_bits, K, nr, &a, &l);
    CHECK(rc == PZ_OK && a == ctx.advice_cells() && l == ctx.lookup_cells(), "tape cell totals == pz_mix_cells");
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
    const std::vector<uint64_t>& tp = ctx.tape();
    bool recs = tp.size() == ns * 4 * L64;
    for (unsigned i = 0; recs && i < K; ++i) {
        const uint64_t* fin = tp.data() + ((size_t)(i + 1) * per - 1) * 4 * L64;
        recs = BigUint::from_limbs(fin, L64) == cts[perm[i]] && BigUint::from_limbs(fin + L64, L64) == pow_mod(rs[i], n, n2) &&
               BigUint::from_limbs(fin + 3 * L64, L64) == res[i] && BigUint::from_limbs(tp.data() + (size_t)i * per * 4 * L64, L64) == rs[i];
    }
    CHECK(recs, "records: every output's chain starts from r_i, its last record is (c_perm(i), r_i^n, q, c'_i)");
    uint64_t *d_work = nullptr, *d_mod = nullptr, *d_adv = nullptr, *d_lk = nullptr;
    std::vector<uint64_t> mod = ctx.modulus().to_limbs(ctx.words());
    bool ok = hipMalloc((void**)&d_work, (ns * 4 + layers * K) * wk * 8 + 64) == hipSuccess && hipMalloc((void**)&d_mod, mod.size() * 8) == hipSuccess &&
              hipMalloc((void**)&d_adv, a * 32) == hipSuccess && hipMalloc((void**)&d_lk, l * 32 + 32) == hipSuccess;
    ok = ok && hipMemcpy(d_mod, mod.data(), mod.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
    size_t a_res = 0, a_eq = 0;
    ok = ok && pz_op_cells(0, 2 * Ln, limb_bits, lookup_bits, &a_res, nullptr) == PZ_OK && pz_op_cells(5, 2 * Ln, limb_bits, lookup_bits, &a_eq, nullptr) == PZ_OK;
    bool bits_one = ok, statement = ok, wrong_zero = ok;
    if (ok) {
        ok = synthesize_mix_circuit(ctx, enc_bits, nr, n, cts, rs, res, wit, d_work, d_mod, d_adv, d_lk) == PZ_OK && pz_sync(ctx.raw()) == PZ_OK;
        for (unsigned i = 0; ok && i < K; ++i) {   // output i's assert_equal_fresh ends (K - 1 - i) result blocks before the stream's end
            uint64_t last[4];
            ok = hipMemcpy(last, d_adv + 4 * (a - 1 - (size_t)(K - 1 - i) * (a_res + a_eq)), 32, hipMemcpyDeviceToHost) == hipSuccess;
            bits_one = bits_one && ok && std::memcmp(last, ONE, 32) == 0;
        }
        // the statement: n | c_1 .. c_K | c'_1 .. c'_K, limb by limb, at the cells pz_mix_public_cells names
        std::vector<uint64_t> cells(Ln + 2 * K * 2 * Ln);
        size_t npub = 0;
        ok = ok && pz_mix_public_cells(Ln, limb_bits, lookup_bits, K, nr, cells.data(), cells.size(), &npub) == PZ_OK;
        statement = ok && npub == cells.size();
        std::vector<BigUint> want_st;
        auto limbs_of = [&](const BigUint& v, unsigned cnt) {
            for (unsigned j = 0; j < cnt; ++j) want_st.push_back((v >> (j * limb_bits)).low_bits(limb_bits));
        };
        limbs_of(n, Ln);
        for (const BigUint& c : cts) limbs_of(c, 2 * Ln);
        for (const BigUint& c : res) limbs_of(c, 2 * Ln);
        for (size_t i = 0; statement && i < npub; ++i) statement = cell_is(ctx, d_adv, cells[i], want_st[i]);
        std::vector<BigUint> wrong = res;
        wrong.back() = wrong.back() + BigUint(1);
        uint64_t last_bad[4] = {1, 1, 1, 1}, first_ok[4] = {0, 0, 0, 0};
        wrong_zero = ok && synthesize_mix_circuit(ctx, enc_bits, nr, n, cts, rs, wrong, wit, d_work, d_mod, d_adv, d_lk) == PZ_OK &&
                     pz_sync(ctx.raw()) == PZ_OK && hipMemcpy(last_bad, d_adv + 4 * (a - 1), 32, hipMemcpyDeviceToHost) == hipSuccess &&
                     hipMemcpy(first_ok, d_adv + 4 * (a - 1 - (size_t)(K - 1) * (a_res + a_eq)), 32, hipMemcpyDeviceToHost) == hipSuccess;
        wrong_zero = wrong_zero && (last_bad[0] | last_bad[1] | last_bad[2] | last_bad[3]) == 0 && (K == 1 || std::memcmp(first_ok, ONE, 32) == 0);
    }
    wit.wipe();
    (void)hipFree(d_work); (void)hipFree(d_mod); (void)hipFree(d_adv); (void)hipFree(d_lk);
    CHECK(ok && bits_one, "device expansion of the mix's tape: every assert_equal_fresh == 1");
    CHECK(ok && statement, "the exposed cells hold n | c_1 .. c_K | c'_1 .. c'_K");
    CHECK(ok && wrong_zero, "a wrong last `res` expands to assert_equal_fresh == 0 for that output alone");
}

static void test_refusals() {
    Context ctx(0);
    RangeChip range{10};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
    const BigUint n = gen_modulus(128);
    auto na = chip.assign_integer(ctx, n, 128).unwrap();
    auto c = chip.assign_integer(ctx, gen_biguint(250), 256).unwrap();
    auto over = chip.assign_integer(ctx, n * n, 256).unwrap();
    auto r = chip.assign_integer(ctx, gen_biguint(120), 128).unwrap();
    CHECK(pc.mix(ctx, na, {c, c, c}, {0, 1, 2}, {r, r, r}, nullptr).err.status == PZ_ERR_INVALID, "mix refuses three ciphertexts");
    CHECK(pc.mix(ctx, na, {c, c}, {0, 1}, {r}, nullptr).err.status == PZ_ERR_INVALID, "mix refuses a missing r");
    CHECK(pc.mix(ctx, na, {c, c}, {0, 0}, {r, r}, nullptr).err.status == PZ_ERR_INVALID, "mix refuses a repeated index");
    CHECK(pc.mix(ctx, na, {c, c}, {0, 2}, {r, r}, nullptr).err.status == PZ_ERR_INVALID, "mix refuses an index >= K");
    CHECK(pc.mix(ctx, na, {c, r}, {0, 1}, {r, r}, nullptr).err.status == PZ_ERR_INVALID, "mix refuses a ciphertext assigned at n's width");
    CHECK(pc.mix(ctx, na, {c, c}, {0, 1}, {r, c}, nullptr).err.status == PZ_ERR_INVALID, "mix refuses an r assigned at full width");
    CHECK(pc.mix(ctx, na, {c, over}, {1, 0}, {r, r}, nullptr).err.status == PZ_ERR_RANGE, "mix refuses a ciphertext of n^2 (PZ_ERR_RANGE)");
}

int main(int argc, char** argv) {
    try {
        test_routing();
        if (!(argc > 1 && std::strcmp(argv[1], "--route-only") == 0)) {
            test_mix(128, 64, 13, 4);
            test_mix(128, 64, 10, 1);
            test_mix(264, 88, 11, 2);
            test_mix(128, 64, 10, 8);
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
