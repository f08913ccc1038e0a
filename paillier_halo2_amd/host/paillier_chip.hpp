// paillier_chip.hpp -- C++ mirror of the reference's chip interface for the hot path, on top of the C ABI
// (include/pz.h).  Rust is not available in this image, the reference is compiled code, so the host side
// above the ABI is C++ with the reference's names, argument meaning and error behaviour:
//
//   reference (Rust)                                          here
//   ------------------------------------------------------    ------------------------------------------
//   halo2_base::Context                                        pz::Context      (device-resident step tape)
//   halo2_base::gates::RangeChip                               pz::RangeChip    {lookup_bits}
//   biguint_halo2::big_uint::chip::BigUintChip                 pz::BigUintChip  ::construct / assign_integer /
//     (call sites paillier.rs:39-57, bench.rs:40-74)             square / refresh / mul_mod / pow_mod_fixed_exp /
//                                                                assert_equal_fresh
//   AssignedBigUint<F, Fresh|Muled>, RefreshAux                pz::AssignedBigUint, pz::RefreshAux
//   paillier.rs:6-9   EncryptionPublicKeyAssigned              pz::EncryptionPublicKeyAssigned
//   paillier.rs:11-20 PaillierChip / construct                 pz::PaillierChip / construct
//   paillier.rs:22-30 get_biguint                              PaillierChip::get_biguint
//   paillier.rs:32-60 encrypt, :62-85 add                      PaillierChip::encrypt / add
//   (add folded over B full-width ciphertexts)                 PaillierChip::tally, pz::paillier_tally_test
//   (c^w and prod c_i^w_i: the scalar homomorphism)            PaillierChip::mul_scalar / weighted_tally, pz::paillier_wtally_test (15.8)
//   (K ciphertexts of small values with a public sum)          PaillierChip::ballot, pz::paillier_ballot_test (15.10)
//   (the same with short randomness, c = g^m hs^s)             PaillierChip::sballot, pz::paillier_sballot_test, pz::djn_generator (15.18)
//   (K choices packed into ONE such ciphertext)                PaillierChip::pballot, pz::paillier_pballot_test, pz::pballot_bases, pz::unpack_tally (15.21)
//   (K ciphertexts shuffled and re-randomised: a mixer's step) pz::benes_route (benes.hpp), PaillierChip::mix, pz::paillier_mix_test (15.17)
//   (the same with short randomness, c' = c_perm hs^s)         PaillierChip::smix, pz::paillier_smix_test (15.20)
//   (the key holder: Dec(c) with the randomness recovered)     pz::PaillierSecretKey, PaillierChip::decrypt, pz::paillier_decrypt_test (15.9)
//   (the same from p and q by the CRT, half-length powers)     PaillierSecretKey::create_crt / has_crt, pz::CrtPath, pz::paillier_decrypt_crt_test (15.22)
//   (T trustees holding additive shares of the exponent)      pz::ThresholdKey, pz::deal_shares, PaillierChip::partial_decrypt / combine (15.11)
//   (any t of T trustees holding Shamir shares of it)          pz::ShamirKey, pz::deal_shamir, PaillierChip::combine_t / mod_inverse (15.12)
//   (the primes every key above starts from)                   PaillierChip::is_probable_prime / prime_search, pz::generate_prime,
//                                                                pz::generate_key, pz::primes_are_safe (15.16)
//   paillier.rs:87-97 paillier_enc_native / _add_native        pz::paillier_enc_native / paillier_add_native
//   bench.rs:11-31    input structs, :33-117 drivers           pz::PaillierEncryptionInput ... paillier_enc_test ...
//
// Where the reference pushes cells into a CPU Context one by one, this Context records a TAPE of the chip
// operations in call order (assign_integer, square, refresh, load_zero, load_constant, mul_mod steps produced by the
// K3 kernels, assert_equal_fresh) with the cells each one pushes, and expands the whole tape to the advice / lookup
// cell streams on the device (synthesize_circuit -> pz_circuit_expand_dev).  Results<> carry plonk::Error's role; unwrap() throws where Rust
// would panic; value mismatches throw like the reference's assert_eq! (paillier.rs:158-163).
#pragma once
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pz.h"
#include "benes.hpp"
#include "biguint.hpp"

namespace pz {

struct Error {  // halo2_proofs::plonk::Error stand-in
    int status = 0;
    std::string msg;
};
template <class T> struct Result {
    bool ok = false;
    T val{};
    Error err;
    static Result Ok(T v) { Result r; r.ok = true; r.val = std::move(v); return r; }
    static Result Err(int st, const std::string& m) { Result r; r.err.status = st; r.err.msg = m; return r; }
    T unwrap() const {
        if (!ok) throw std::runtime_error("called unwrap() on an Err: " + err.msg);  // Rust: panic
        return val;
    }
};

struct RangeChip {
    unsigned lookup_bits;
};

// device context: owns the pz_ctx and the step tape of the circuit being built
class Context {
  public:
    explicit Context(int device = 0) {
        int dev = device;
        int rc = pz_init(1, &dev, &ctx_);
        if (rc != PZ_OK) throw std::runtime_error(std::string("pz_init: ") + pz_strerror(rc));
    }
    ~Context() { if (ctx_) pz_free(ctx_); }
    Context(const Context&) = delete;
    pz_ctx* raw() { return ctx_; }
    // ---- the operation tape: what the reference's Context would hold, operation by operation
    // (0 .. 5 are pz_op_cells' operations; the three after them push a cell count of their own: record_cells)
    enum Op { ASSIGN = 0, SQUARE = 1, REFRESH = 2, CONST_CELL = 3, MUL_MOD = 4, ASSERT_EQUAL = 5, LOAD_WITNESS = 6, NUM_TO_BITS = 7, SELECT = 8,
              SUM = 9, SWITCH = 10 };
    struct OpRec {
        Op op;
        unsigned limbs;      // limb count the operation works on
        size_t count;        // MUL_MOD: number of steps; otherwise 1
    };
    void set_shape(unsigned limb_bits, unsigned lookup_bits) { W_ = limb_bits; lookup_bits_ = lookup_bits; }
    // record an operation and the cells it pushes (pz_op_cells: the same arithmetic pz_circuit_cells sums)
    void record(Op op, unsigned limbs, size_t count = 1) {
        size_t a = 0, l = 0;
        int rc = pz_op_cells((int)op, limbs, W_, lookup_bits_, &a, &l);
        if (rc != PZ_OK) throw std::runtime_error(std::string("pz_op_cells: ") + pz_strerror(rc));
        advice_cells_ += a * count;
        lookup_cells_ += l * count;
        if (!ops_.empty() && ops_.back().op == op && op == MUL_MOD && ops_.back().limbs == limbs) ops_.back().count += count;
        else ops_.push_back(OpRec{op, limbs, count});
    }
    // an operation of the weighted tally that pz_op_cells does not know: `cells` advice cells, no lookups
    void record_cells(Op op, unsigned limbs, size_t cells) {
        advice_cells_ += cells;
        ops_.push_back(OpRec{op, limbs, 1});
    }
    size_t load_witness() { record_cells(LOAD_WITNESS, 1, 1); return witness_cells_++; }   // ctx.load_witness(v): one advice cell, no gate
    void sum(size_t terms) { record_cells(SUM, 1, 1 + 3 * (terms - 1)); }         // FlexGate::sum over `terms` >= 2 cells: a | 1 | b | a + b | ..
    // one switch of the mix's network over `limbs`-limb integers: assert_bit's [0, b, b, b], then per limb two selects of 8 cells
    void conditional_swap(unsigned limbs) { record_cells(SWITCH, limbs, 4 + 16 * (size_t)limbs); }
    size_t load_zero() { record(CONST_CELL, 1); return zero_cells_++; }            // paillier.rs:47 ctx.load_zero(): one advice cell
    size_t load_constant_one() { record(CONST_CELL, 1); return zero_cells_++; }    // assign_constant(1) of pow_mod_fixed_exp
    const std::vector<OpRec>& ops() const { return ops_; }
    size_t advice_cells() const { return advice_cells_; }
    size_t lookup_cells() const { return lookup_cells_; }
    unsigned lookup_bits() const { return lookup_bits_; }
    // tape of mul_mod steps in emission order: (a|b|q|r), `words` 64-bit words each, whatever the circuit's limb
    // width is; all steps of one circuit share the limb count, the limb width and the modulus
    void push_steps(const std::vector<uint64_t>& steps, unsigned words, unsigned limbs, unsigned limb_bits, const BigUint& modulus) {
        if (L_ && (L_ != limbs || W_ != limb_bits || modulus_ != modulus)) throw std::logic_error("one Context holds steps of one modulus");
        L_ = limbs;
        W_ = limb_bits;
        words_ = words;
        modulus_ = modulus;
        tape_.insert(tape_.end(), steps.begin(), steps.end());
        record(MUL_MOD, limbs, steps.size() / (4 * (size_t)words));
    }
    size_t n_steps() const { return words_ ? tape_.size() / (4 * words_) : 0; }
    const std::vector<uint64_t>& tape() const { return tape_; }
    unsigned limbs() const { return L_; }        // circuit limbs per big integer
    unsigned limb_bits() const { return W_; }
    unsigned words() const { return words_; }    // 64-bit words per big integer of a step record
    const BigUint& modulus() const { return modulus_; }

  private:
    pz_ctx* ctx_ = nullptr;
    size_t zero_cells_ = 0, witness_cells_ = 0, advice_cells_ = 0, lookup_cells_ = 0;
    unsigned L_ = 0, W_ = 64, words_ = 0, lookup_bits_ = 0;
    std::vector<OpRec> ops_;
    BigUint modulus_;
    std::vector<uint64_t> tape_;
};

struct Fresh {};
struct Muled {};

struct RefreshAux {   // paillier.rs:40-44
    unsigned limb_bits, num_limbs_l, num_limbs_r;
    std::vector<uint8_t> increased_limbs_vec;   // extra limbs each product limb's maximal value spills into
    static RefreshAux new_(unsigned limb_bits, unsigned l, unsigned r) {
        RefreshAux a{limb_bits, l, r, std::vector<uint8_t>(256)};
        uint32_t n = 0;
        int rc = pz_refresh_aux(limb_bits, l, r, a.increased_limbs_vec.data(), 256, &n);
        if (rc != PZ_OK) throw std::runtime_error(std::string("RefreshAux::new: ") + pz_strerror(rc));
        a.increased_limbs_vec.resize(n);
        return a;
    }
};

template <class Kind> class AssignedBigUint {
  public:
    AssignedBigUint() {}
    AssignedBigUint(BigUint v, unsigned num_limbs, unsigned max_limb_bits)
        : value_(std::move(v)), num_limbs_(num_limbs), max_limb_bits_(max_limb_bits) {}
    const BigUint& value() const { return value_; }
    unsigned num_limbs() const { return num_limbs_; }
    unsigned max_limb_bits() const { return max_limb_bits_; }
    // the circuit's limbs (max_limb_bits wide, limbs()[0] least significant): what the reference's limbs() cells hold
    std::vector<BigUint> limbs() const {
        if (value_.bits() > (size_t)num_limbs_ * max_limb_bits_) throw std::range_error("integer does not fit the limb count");
        std::vector<BigUint> r;
        for (unsigned i = 0; i < num_limbs_; ++i) r.push_back((value_ >> ((size_t)i * max_limb_bits_)).low_bits(max_limb_bits_));
        return r;
    }
    // the same integer as the C ABI takes it: little-endian 64-bit words covering num_limbs * max_limb_bits bits
    unsigned num_words() const { return (num_limbs_ * max_limb_bits_ + 63) / 64; }
    std::vector<uint64_t> words() const {
        if (value_.bits() > (size_t)num_limbs_ * max_limb_bits_) throw std::range_error("integer does not fit the limb count");
        return value_.to_limbs(num_words());
    }
    AssignedBigUint extend_limbs(unsigned extra, size_t /*zero_cell*/) const {   // paillier.rs:49,53,79-80
        return AssignedBigUint(value_, num_limbs_ + extra, max_limb_bits_);
    }

  private:
    BigUint value_;
    unsigned num_limbs_ = 0, max_limb_bits_ = 64;
};

class BigUintChip {
  public:
    const RangeChip* range;
    unsigned limb_bits;
    static BigUintChip construct(const RangeChip* range, unsigned limb_bits) {
        if (limb_bits < 16 || limb_bits > 90) throw std::invalid_argument("limb_bits outside 16..90 (K4 carries a limb in two 64-bit words)");
        return BigUintChip{range, limb_bits};
    }
    // assign_integer(ctx, Value::known(v), bit_len): bit_len must be a multiple of limb_bits, v must fit (its limbs'
    // range checks would fail otherwise); pushes the limbs and one range check each
    Result<AssignedBigUint<Fresh>> assign_integer(Context& ctx, const BigUint& v, unsigned bit_len) const {
        if (bit_len % limb_bits) return Result<AssignedBigUint<Fresh>>::Err(PZ_ERR_INVALID, "bit_len % limb_bits != 0");
        if (v.bits() > bit_len) return Result<AssignedBigUint<Fresh>>::Err(PZ_ERR_RANGE, "value exceeds bit_len");
        ctx.set_shape(limb_bits, range->lookup_bits);
        ctx.record(Context::ASSIGN, bit_len / limb_bits);
        return Result<AssignedBigUint<Fresh>>::Ok(AssignedBigUint<Fresh>(v, bit_len / limb_bits, limb_bits));
    }
    // square = mul(a, a): unreduced limb products (2 l - 1 limbs of up to 2 W + log2(l) bits); the cells are the limb
    // convolution K4 writes on the device
    Result<AssignedBigUint<Muled>> square(Context& ctx, const AssignedBigUint<Fresh>& a) const {  // paillier.rs:39
        ctx.record(Context::SQUARE, a.num_limbs());
        unsigned lg = 0;
        while ((1u << lg) < a.num_limbs()) ++lg;
        return Result<AssignedBigUint<Muled>>::Ok(AssignedBigUint<Muled>(a.value() * a.value(), 2 * a.num_limbs() - 1,
                                                                         2 * limb_bits + lg));
    }
    // refresh: cut every product limb back to limb_bits-wide limbs, carrying into the limbs above as aux says
    Result<AssignedBigUint<Fresh>> refresh(Context& ctx, const AssignedBigUint<Muled>& a, const RefreshAux& aux) const {  // :45
        using R = Result<AssignedBigUint<Fresh>>;
        if (aux.limb_bits != limb_bits) return R::Err(PZ_ERR_INVALID, "refresh: aux.limb_bits != limb_bits");
        if (a.num_limbs() != aux.num_limbs_l + aux.num_limbs_r - 1) return R::Err(PZ_ERR_INVALID, "refresh: limb count does not match aux");
        if (aux.num_limbs_l != aux.num_limbs_r) return R::Err(PZ_ERR_UNSUPPORTED, "refresh: only squares are expanded on the device");
        const unsigned fresh = (unsigned)aux.increased_limbs_vec.size();
        if (a.value().bits() > (size_t)fresh * limb_bits) return R::Err(PZ_ERR_RANGE, "refresh: value exceeds the refreshed limbs");
        ctx.record(Context::REFRESH, aux.num_limbs_l);
        return R::Ok(AssignedBigUint<Fresh>(a.value(), fresh, limb_bits));
    }
    // mul_mod(ctx, a, b, n): witness (q, r) from the K3 kernel, step recorded for K4
    Result<AssignedBigUint<Fresh>> mul_mod(Context& ctx, const AssignedBigUint<Fresh>& a, const AssignedBigUint<Fresh>& b,
                                           const AssignedBigUint<Fresh>& n) const {
        const unsigned L = n.num_limbs();
        if (a.num_limbs() != L || b.num_limbs() != L) return Result<AssignedBigUint<Fresh>>::Err(PZ_ERR_INVALID, "limb count mismatch");
        const unsigned Wd = n.num_words();
        std::vector<uint64_t> av = a.words(), bv = b.words(), nv = n.words(), q(Wd), r(Wd);
        int rc = pz_mul_mod(ctx.raw(), Wd, av.data(), bv.data(), nv.data(), q.data(), r.data());
        if (rc != PZ_OK) return Result<AssignedBigUint<Fresh>>::Err(rc, std::string("pz_mul_mod: ") + pz_strerror(rc));
        BigUint qv = BigUint::from_limbs(q.data(), Wd);
        if (qv.bits() > (size_t)L * limb_bits)   // the circuit assigns q with L limbs: its range check would fail
            return Result<AssignedBigUint<Fresh>>::Err(PZ_ERR_RANGE, "quotient does not fit the assigned limb count");
        std::vector<uint64_t> step;
        step.insert(step.end(), av.begin(), av.end());
        step.insert(step.end(), bv.begin(), bv.end());
        step.insert(step.end(), q.begin(), q.end());
        step.insert(step.end(), r.begin(), r.end());
        ctx.push_steps(step, Wd, L, limb_bits, n.value());
        return Result<AssignedBigUint<Fresh>>::Ok(AssignedBigUint<Fresh>(BigUint::from_limbs(r.data(), Wd), L, limb_bits));
    }
    // pow_mod_fixed_exp(ctx, a, e, n): e is a native BigUint -- the exponent's bits shape the circuit
    Result<AssignedBigUint<Fresh>> pow_mod_fixed_exp(Context& ctx, const AssignedBigUint<Fresh>& a, const BigUint& e,
                                                     const AssignedBigUint<Fresh>& n) const {
        const unsigned L = n.num_limbs();
        if (a.num_limbs() != L) return Result<AssignedBigUint<Fresh>>::Err(PZ_ERR_INVALID, "limb count mismatch");
        (void)ctx.load_constant_one();   // acc = assign_constant(1) ...
        (void)ctx.load_zero();           // ... extended with the zero cell
        const unsigned Wd = n.num_words();
        std::vector<uint64_t> av = a.words(), nv = n.words(), res(Wd);
        const unsigned el = e.l.empty() ? 1 : (unsigned)e.l.size();
        std::vector<uint64_t> ev = e.to_limbs(el);
        size_t cap = e.bits();
        for (uint64_t w : ev) cap += (size_t)__builtin_popcountll(w);
        std::vector<uint64_t> steps(std::max<size_t>(cap, 1) * 4 * Wd);
        size_t ns = cap;
        int rc = pz_paillier_trace(ctx.raw(), Wd, nv.data(), av.data(), ev.data(), el, steps.data(), &ns, res.data());
        if (rc != PZ_OK) return Result<AssignedBigUint<Fresh>>::Err(rc, std::string("pz_paillier_trace: ") + pz_strerror(rc));
        steps.resize(ns * 4 * Wd);
        if (ns) ctx.push_steps(steps, Wd, L, limb_bits, n.value());
        return Result<AssignedBigUint<Fresh>>::Ok(AssignedBigUint<Fresh>(BigUint::from_limbs(res.data(), Wd), L, limb_bits));
    }
    // is_equal_fresh limb by limb (load_zero, load_constant(1), is_equal + and per limb), result constrained to 1
    Result<bool> assert_equal_fresh(Context& ctx, const AssignedBigUint<Fresh>& a, const AssignedBigUint<Fresh>& b) const {
        const unsigned max_n = std::max(a.num_limbs(), b.num_limbs());
        ctx.record(Context::ASSERT_EQUAL, max_n);
        std::vector<BigUint> al = a.extend_limbs(max_n - a.num_limbs(), 0).limbs(), bl = b.extend_limbs(max_n - b.num_limbs(), 0).limbs();
        bool eq = true;
        for (unsigned i = 0; i < max_n; ++i) eq = eq && al[i] == bl[i];
        if (!eq) return Result<bool>::Err(PZ_ERR_INVALID, "assert_equal_fresh: constraint not satisfied");
        return Result<bool>::Ok(true);
    }
};

// a weight of the weighted tally: the value ctx.load_witness put into one advice cell
struct AssignedWeight {
    uint64_t value = 0;
    size_t cell = 0;
};

// The key holder's secret key as a device handle (pz_paillier_sk_create: validated there; lambda, d and mu stay on the device and are
// overwritten when the handle goes).  d = n^-1 mod lambda is the caller's.
class PaillierSecretKey {
  public:
    static Result<std::shared_ptr<PaillierSecretKey>> create(Context& ctx, const BigUint& n, const BigUint& g, const BigUint& lambda,
                                                             const BigUint& d) {
        using R = Result<std::shared_ptr<PaillierSecretKey>>;
        const size_t Ln = std::max<size_t>(1, n.l.size());
        if (g.l.size() > Ln || lambda.l.size() > Ln || d.l.size() > Ln) return R::Err(PZ_ERR_INVALID, "a key value is wider than n");
        std::vector<uint64_t> nv = n.to_limbs(Ln), gv = g.to_limbs(Ln), lv = lambda.to_limbs(Ln), dv = d.to_limbs(Ln);
        pz_paillier_sk* h = nullptr;
        int rc = pz_paillier_sk_create(ctx.raw(), (uint32_t)Ln, nv.data(), gv.data(), lv.data(), dv.data(), &h);
        std::fill(lv.begin(), lv.end(), 0);
        std::fill(dv.begin(), dv.end(), 0);
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_paillier_sk_create: ") + pz_strerror(rc));
        return R::Ok(std::shared_ptr<PaillierSecretKey>(new PaillierSecretKey(ctx.raw(), h, (unsigned)Ln, n, g)));
    }
    // the same with the primes (pz_paillier_sk_create_crt): the handle serves the CRT path as well.  p and q
    // may come in either order; primality is not tested there (pz_bigint_is_prime is the caller's).
    static Result<std::shared_ptr<PaillierSecretKey>> create_crt(Context& ctx, const BigUint& n, const BigUint& g, const BigUint& lambda,
                                                                 const BigUint& d, const BigUint& p, const BigUint& q) {
        using R = Result<std::shared_ptr<PaillierSecretKey>>;
        const size_t Ln = std::max<size_t>(1, n.l.size());
        if (g.l.size() > Ln || lambda.l.size() > Ln || d.l.size() > Ln || p.l.size() > Ln || q.l.size() > Ln)
            return R::Err(PZ_ERR_INVALID, "a key value is wider than n");
        std::vector<uint64_t> nv = n.to_limbs(Ln), gv = g.to_limbs(Ln), lv = lambda.to_limbs(Ln), dv = d.to_limbs(Ln), pv = p.to_limbs(Ln),
                              qv = q.to_limbs(Ln);
        pz_paillier_sk* h = nullptr;
        int rc = pz_paillier_sk_create_crt(ctx.raw(), (uint32_t)Ln, nv.data(), gv.data(), lv.data(), dv.data(), pv.data(), qv.data(), &h);
        for (auto* v : {&lv, &dv, &pv, &qv}) std::fill(v->begin(), v->end(), 0);
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_paillier_sk_create_crt: ") + pz_strerror(rc));
        return R::Ok(std::shared_ptr<PaillierSecretKey>(new PaillierSecretKey(ctx.raw(), h, (unsigned)Ln, n, g)));
    }
    bool has_crt() const { return pz_paillier_sk_has_crt(sk_) == 1; }
    ~PaillierSecretKey() { (void)pz_paillier_sk_free(ctx_, sk_); }
    PaillierSecretKey(const PaillierSecretKey&) = delete;
    const pz_paillier_sk* raw() const { return sk_; }
    unsigned words() const { return Ln_; }
    const BigUint& n() const { return n_; }
    const BigUint& g() const { return g_; }

  private:
    PaillierSecretKey(pz_ctx* c, pz_paillier_sk* h, unsigned Ln, const BigUint& n, const BigUint& g) : ctx_(c), sk_(h), Ln_(Ln), n_(n), g_(g) {}
    pz_ctx* ctx_;
    pz_paillier_sk* sk_;
    unsigned Ln_;
    BigUint n_, g_;
};
// which path PaillierChip::decrypt takes
enum class CrtPath { No, Yes, Auto };
// one decryption: the plaintext, the randomness with c = g^m r^n mod n^2, and whether c was a unit at all (if not, m = r = 0)
struct Decryption {
    BigUint m, r;
    bool unit = false;
};

// T-of-T threshold decryption.  The PUBLIC threshold key: hs[i] = v^theta_i mod n^2 is what trustee i's proofs
// (circuit kind 7) are checked against, mu2 = (2a)^-1 mod n with 1 + a n = g^theta mod n^2 is the combiner's last factor
struct ThresholdKey {
    BigUint n, g, v;
    std::vector<BigUint> hs;
    BigUint mu2;
    bool v_order_proved = false;   // the dealer checked ord v = n lambda / 2 (it can for safe primes only)
};
// one trustee's answer: h = v^theta (equal to its hs entry) and u_j = (c_j^2)^theta mod n^2
struct PartialDecryption {
    BigUint h;
    std::vector<BigUint> us;
};
// t-of-T threshold decryption.  The PUBLIC key: hs[i - 1] = v^(s_i) mod n^2 for trustee i's Shamir share s_i,
// mu2 = (2 a trustees!)^-1 mod n the last factor of PaillierChip::combine_t over any `threshold` of the partials
struct ShamirKey {
    BigUint n, g, v;
    std::vector<BigUint> hs;
    BigUint mu2;
    size_t trustees = 0, threshold = 0;
    bool v_order_proved = false;
};

struct EncryptionPublicKeyAssigned {  // paillier.rs:6-9
    AssignedBigUint<Fresh> n, g;
};

class PaillierChip {  // paillier.rs:11-15
  public:
    const BigUintChip* biguint;
    unsigned enc_bits;  // stored, never read by encrypt/add -- as in the reference
    static PaillierChip construct(const BigUintChip* biguint, unsigned enc_bits) { return PaillierChip{biguint, enc_bits}; }

    // paillier.rs:22-30: fold limbs MSB -> LSB with shift max_limb_bits
    BigUint get_biguint(const AssignedBigUint<Fresh>& assigned) const {
        BigUint acc;
        std::vector<BigUint> limbs = assigned.limbs();
        for (size_t i = limbs.size(); i-- > 0;) acc = (acc << assigned.max_limb_bits()) + limbs[i];
        return acc;
    }

    // paillier.rs:32-60
    Result<AssignedBigUint<Fresh>> encrypt(Context& ctx, const EncryptionPublicKeyAssigned& pk_enc, const AssignedBigUint<Fresh>& m,
                                           const AssignedBigUint<Fresh>& r) const {
        using R = Result<AssignedBigUint<Fresh>>;
        auto n2m = biguint->square(ctx, pk_enc.n);
        if (!n2m.ok) return R::Err(n2m.err.status, n2m.err.msg);
        RefreshAux aux = RefreshAux::new_(biguint->limb_bits, pk_enc.n.num_limbs(), pk_enc.n.num_limbs());
        auto n2r = biguint->refresh(ctx, n2m.val, aux);
        if (!n2r.ok) return R::Err(n2r.err.status, n2r.err.msg);
        const AssignedBigUint<Fresh>& n2 = n2r.val;
        size_t zero_value = ctx.load_zero();
        auto g_extended = pk_enc.g.extend_limbs(n2.num_limbs() - pk_enc.g.num_limbs(), zero_value);
        BigUint m_biguint = get_biguint(m);
        auto gm = biguint->pow_mod_fixed_exp(ctx, g_extended, m_biguint, n2);
        if (!gm.ok) return gm;
        auto r_extended = r.extend_limbs(n2.num_limbs() - r.num_limbs(), zero_value);
        BigUint n_biguint = get_biguint(pk_enc.n);
        auto rn = biguint->pow_mod_fixed_exp(ctx, r_extended, n_biguint, n2);
        if (!rn.ok) return rn;
        return biguint->mul_mod(ctx, gm.val, rn.val, n2);
    }

    // paillier.rs:62-85 (pk_enc.g unused, as in the reference)
    Result<AssignedBigUint<Fresh>> add(Context& ctx, const EncryptionPublicKeyAssigned& pk_enc, const AssignedBigUint<Fresh>& c1,
                                       const AssignedBigUint<Fresh>& c2) const {
        using R = Result<AssignedBigUint<Fresh>>;
        auto n2m = biguint->square(ctx, pk_enc.n);
        if (!n2m.ok) return R::Err(n2m.err.status, n2m.err.msg);
        RefreshAux aux = RefreshAux::new_(biguint->limb_bits, pk_enc.n.num_limbs(), pk_enc.n.num_limbs());
        auto n2r = biguint->refresh(ctx, n2m.val, aux);
        if (!n2r.ok) return R::Err(n2r.err.status, n2r.err.msg);
        const AssignedBigUint<Fresh>& n2 = n2r.val;
        size_t zero_value = ctx.load_zero();
        auto c1e = c1.extend_limbs(n2.num_limbs() - c1.num_limbs(), zero_value);
        auto c2e = c2.extend_limbs(n2.num_limbs() - c2.num_limbs(), zero_value);
        return biguint->mul_mod(ctx, c1e, c2e, n2);
    }

    // The tally: prod cts mod n^2 -- `add` folded over FULL-WIDTH ciphertexts (n2.num_limbs() limbs each, so
    // nothing is extended and there is no load_zero), n^2 hoisted once as encrypt does (paillier.rs:39-45), the products in
    // pz_paillier_tally's tree order: level by level the neighbours of the current list, an odd last element carried up.
    Result<AssignedBigUint<Fresh>> tally(Context& ctx, const EncryptionPublicKeyAssigned& pk_enc,
                                         const std::vector<AssignedBigUint<Fresh>>& cts) const {
        using R = Result<AssignedBigUint<Fresh>>;
        if (cts.size() < 2) return R::Err(PZ_ERR_INVALID, "tally: fewer than two ciphertexts");
        auto n2m = biguint->square(ctx, pk_enc.n);
        if (!n2m.ok) return R::Err(n2m.err.status, n2m.err.msg);
        RefreshAux aux = RefreshAux::new_(biguint->limb_bits, pk_enc.n.num_limbs(), pk_enc.n.num_limbs());
        auto n2r = biguint->refresh(ctx, n2m.val, aux);
        if (!n2r.ok) return R::Err(n2r.err.status, n2r.err.msg);
        const AssignedBigUint<Fresh>& n2 = n2r.val;
        const unsigned L = n2.num_limbs(), Wd = n2.num_words(), wn = pk_enc.n.num_words(), wk = 2 * wn;   // K3 works on 2 * wn words
        std::vector<uint64_t> nv = pk_enc.n.words(), cv;
        for (const auto& c : cts) {
            if (c.num_limbs() != L) return R::Err(PZ_ERR_INVALID, "tally: a ciphertext is not assigned at full width");
            std::vector<uint64_t> w = c.value().to_limbs(wk);
            cv.insert(cv.end(), w.begin(), w.end());
        }
        const size_t ns = cts.size() - 1;
        std::vector<uint64_t> rec(ns * 4 * wk), root(wk);
        int rc = pz_paillier_tally(ctx.raw(), wn, cts.size(), nv.data(), cv.data(), rec.data(), ns, root.data());
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_paillier_tally: ") + pz_strerror(rc));
        // the tape holds Wd words per integer (Wd < 2 * wn where limb_bits does not divide 64: the words above are zero)
        std::vector<uint64_t> steps;
        for (size_t f = 0; f < ns * 4; ++f) {
            if (BigUint::from_limbs(rec.data() + f * wk, wk).bits() > (size_t)L * biguint->limb_bits)
                return R::Err(PZ_ERR_RANGE, "a step's integer does not fit the assigned limb count");
            steps.insert(steps.end(), rec.begin() + f * wk, rec.begin() + f * wk + Wd);
        }
        ctx.push_steps(steps, Wd, L, biguint->limb_bits, n2.value());
        return R::Ok(AssignedBigUint<Fresh>(BigUint::from_limbs(root.data(), wk), L, biguint->limb_bits));
    }

    // The weighted tally: prod cts[i]^weights[i] mod n^2 = Enc(sum w_i m_i).  n^2 hoisted once; per ciphertext
    // BigUintChip::pow_mod over w_bits in-circuit bits -- assign_constant(1), load_zero, num_to_bits(w_i, w_bits), then per bit
    // mul_mod(acc, sq), the limb-wise select, square_mod(sq) --; then the tally's product tree over the powers (one ciphertext: none).
    // One pz_paillier_wtally call computes every record; the tape takes them in the circuit's order.
    Result<AssignedBigUint<Fresh>> weighted_tally(Context& ctx, const EncryptionPublicKeyAssigned& pk_enc,
                                                  const std::vector<AssignedBigUint<Fresh>>& cts, const std::vector<AssignedWeight>& weights,
                                                  unsigned w_bits) const {
        using R = Result<AssignedBigUint<Fresh>>;
        if (cts.empty() || cts.size() != weights.size()) return R::Err(PZ_ERR_INVALID, "weighted_tally: one weight per ciphertext, at least one");
        if (w_bits < 1 || w_bits > 64) return R::Err(PZ_ERR_INVALID, "weighted_tally: w_bits outside 1 .. 64");
        auto n2m = biguint->square(ctx, pk_enc.n);
        if (!n2m.ok) return R::Err(n2m.err.status, n2m.err.msg);
        RefreshAux aux = RefreshAux::new_(biguint->limb_bits, pk_enc.n.num_limbs(), pk_enc.n.num_limbs());
        auto n2r = biguint->refresh(ctx, n2m.val, aux);
        if (!n2r.ok) return R::Err(n2r.err.status, n2r.err.msg);
        const AssignedBigUint<Fresh>& n2 = n2r.val;
        const unsigned L = n2.num_limbs(), Wd = n2.num_words(), wn = pk_enc.n.num_words(), wk = 2 * wn;   // K3 works on 2 * wn words
        std::vector<uint64_t> nv = pk_enc.n.words(), cv, wv;
        for (const auto& c : cts) {
            if (c.num_limbs() != L) return R::Err(PZ_ERR_INVALID, "weighted_tally: a ciphertext is not assigned at full width");
            std::vector<uint64_t> w = c.value().to_limbs(wk);
            cv.insert(cv.end(), w.begin(), w.end());
        }
        for (const AssignedWeight& w : weights) wv.push_back(w.value);
        const size_t B = cts.size(), n_chain = 2 * B * w_bits, ns = n_chain + B - 1;
        std::vector<uint64_t> rec(ns * 4 * wk), root(wk);
        int rc = pz_paillier_wtally(ctx.raw(), wn, B, w_bits, nv.data(), cv.data(), wv.data(), rec.data(), ns, root.data());
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_paillier_wtally: ") + pz_strerror(rc));
        // the tape holds Wd words per integer (Wd < 2 * wn where limb_bits does not divide 64: the words above are zero)
        auto steps_of = [&](size_t first, size_t count, std::vector<uint64_t>& out) {
            out.clear();
            for (size_t f = first * 4; f < (first + count) * 4; ++f) {
                if (BigUint::from_limbs(rec.data() + f * wk, wk).bits() > (size_t)L * biguint->limb_bits) return false;
                out.insert(out.end(), rec.begin() + f * wk, rec.begin() + f * wk + Wd);
            }
            return true;
        };
        std::vector<uint64_t> steps;
        for (size_t i = 0; i < B; ++i) {
            (void)ctx.load_constant_one();
            (void)ctx.load_zero();
            ctx.record_cells(Context::NUM_TO_BITS, 1, 7 * (size_t)w_bits - 2);
            for (unsigned j = 0; j < w_bits; ++j) {
                const size_t at = 2 * (i * w_bits + j);
                if (!steps_of(at, 1, steps)) return R::Err(PZ_ERR_RANGE, "a step's integer does not fit the assigned limb count");
                ctx.push_steps(steps, Wd, L, biguint->limb_bits, n2.value());
                ctx.record_cells(Context::SELECT, L, 8 * (size_t)L);
                if (!steps_of(at + 1, 1, steps)) return R::Err(PZ_ERR_RANGE, "a step's integer does not fit the assigned limb count");
                ctx.push_steps(steps, Wd, L, biguint->limb_bits, n2.value());
            }
        }
        if (B > 1) {
            if (!steps_of(n_chain, B - 1, steps)) return R::Err(PZ_ERR_RANGE, "a step's integer does not fit the assigned limb count");
            ctx.push_steps(steps, Wd, L, biguint->limb_bits, n2.value());
        }
        return R::Ok(AssignedBigUint<Fresh>(BigUint::from_limbs(root.data(), wk), L, biguint->limb_bits));
    }

    // The ballot: c_i = g^m_i r_i^n mod n^2 for K messages under one key.  n^2 hoisted once, load_zero; per
    // ciphertext pow_mod(g_ext, m_i) over m_bits in-circuit bits (the weighted tally's chain, the trailing square kept),
    // pow_mod_fixed_exp(r_i_ext, n) and the final mul_mod.  One pz_paillier_ballot call computes every record; the tape takes them in the
    // circuit's order, which is the call's.  The messages' load_witness cells, their sum and the r_i are assigned by the caller
    // (paillier_ballot_test), in front of this.
    Result<std::vector<AssignedBigUint<Fresh>>> ballot(Context& ctx, const EncryptionPublicKeyAssigned& pk_enc, const std::vector<AssignedWeight>& ms,
                                                       const std::vector<AssignedBigUint<Fresh>>& rs, unsigned m_bits) const {
        using R = Result<std::vector<AssignedBigUint<Fresh>>>;
        if (ms.empty() || ms.size() != rs.size() || ms.size() > 1024) return R::Err(PZ_ERR_INVALID, "ballot: one r per message, 1 .. 1024 of them");
        if (m_bits < 1 || m_bits > 64) return R::Err(PZ_ERR_INVALID, "ballot: m_bits outside 1 .. 64");
        auto n2m = biguint->square(ctx, pk_enc.n);
        if (!n2m.ok) return R::Err(n2m.err.status, n2m.err.msg);
        RefreshAux aux = RefreshAux::new_(biguint->limb_bits, pk_enc.n.num_limbs(), pk_enc.n.num_limbs());
        auto n2r = biguint->refresh(ctx, n2m.val, aux);
        if (!n2r.ok) return R::Err(n2r.err.status, n2r.err.msg);
        const AssignedBigUint<Fresh>& n2 = n2r.val;
        (void)ctx.load_zero();
        const unsigned L = n2.num_limbs(), Wd = n2.num_words(), wn = pk_enc.n.num_words(), wk = 2 * wn;   // K3 works on 2 * wn words
        std::vector<uint64_t> nv = pk_enc.n.words(), gv = pk_enc.g.value().to_limbs(wn), mv, rv;
        for (const AssignedWeight& m : ms) mv.push_back(m.value);
        for (const auto& r : rs) {
            if (r.num_limbs() != pk_enc.n.num_limbs()) return R::Err(PZ_ERR_INVALID, "ballot: an r is not assigned at n's width");
            std::vector<uint64_t> w = r.value().to_limbs(wn);
            rv.insert(rv.end(), w.begin(), w.end());
        }
        const BigUint n_biguint = get_biguint(pk_enc.n);
        size_t nr = n_biguint.bits();
        for (uint64_t w : nv) nr += (size_t)__builtin_popcountll(w);
        const size_t K = ms.size(), per = 2 * (size_t)m_bits + nr + 1;
        std::vector<uint64_t> rec(K * per * 4 * wk), cv(K * wk);
        uint32_t nr_lib = 0;
        int rc = pz_paillier_ballot(ctx.raw(), wn, K, m_bits, nv.data(), gv.data(), mv.data(), rv.data(), rec.data(), K * per, &nr_lib, cv.data());
        std::fill(mv.begin(), mv.end(), 0);
        std::fill(rv.begin(), rv.end(), 0);
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_paillier_ballot: ") + pz_strerror(rc));
        if (nr_lib != nr) return R::Err(PZ_ERR_INTERNAL, "ballot: the library counts another r^n chain");
        // the tape holds Wd words per integer (Wd < 2 * wn where limb_bits does not divide 64: the words above are zero)
        auto steps_of = [&](size_t first, size_t count, std::vector<uint64_t>& out) {
            out.clear();
            for (size_t f = first * 4; f < (first + count) * 4; ++f) {
                if (BigUint::from_limbs(rec.data() + f * wk, wk).bits() > (size_t)L * biguint->limb_bits) return false;
                out.insert(out.end(), rec.begin() + f * wk, rec.begin() + f * wk + Wd);
            }
            return true;
        };
        const char* wide = "a step's integer does not fit the assigned limb count";
        std::vector<uint64_t> steps;
        std::vector<AssignedBigUint<Fresh>> out;
        for (size_t i = 0; i < K; ++i) {
            (void)ctx.load_constant_one();
            (void)ctx.load_zero();
            ctx.record_cells(Context::NUM_TO_BITS, 1, 7 * (size_t)m_bits - 2);
            for (unsigned j = 0; j < m_bits; ++j) {
                const size_t at = i * per + 2 * j;
                if (!steps_of(at, 1, steps)) return R::Err(PZ_ERR_RANGE, wide);
                ctx.push_steps(steps, Wd, L, biguint->limb_bits, n2.value());
                ctx.record_cells(Context::SELECT, L, 8 * (size_t)L);
                if (!steps_of(at + 1, 1, steps)) return R::Err(PZ_ERR_RANGE, wide);
                ctx.push_steps(steps, Wd, L, biguint->limb_bits, n2.value());
            }
            (void)ctx.load_constant_one();
            (void)ctx.load_zero();
            if (!steps_of(i * per + 2 * m_bits, nr + 1, steps)) return R::Err(PZ_ERR_RANGE, wide);   // the r^n chain, then the final block
            ctx.push_steps(steps, Wd, L, biguint->limb_bits, n2.value());
            out.push_back(AssignedBigUint<Fresh>(BigUint::from_limbs(cv.data() + i * wk, wk), L, biguint->limb_bits));
        }
        std::fill(rec.begin(), rec.end(), 0);
        return R::Ok(out);
    }

    // The short-randomness ballot: c_i = g^m_i hs^s_i mod n^2 for K messages under one key whose hs = h^n mod
    // n^2 is public (pz::djn_generator).  n^2 hoisted once, load_zero; per ciphertext pow_mod(g_ext, m_i) over m_bits in-circuit bits as
    // ballot does, pow_mod(hs, s_i) as kind 7 emits a chain -- [1, 0], then per limb of s_i num_to_bits and that limb's blocks -- and the
    // final mul_mod.  One pz_paillier_sballot call computes every record; the tape takes them in the circuit's order, which is the
    // call's.  hs, the messages' load_witness cells, their sum and the s_i (all of ONE limb count, 1 .. 2 * n's) are assigned by the
    // caller (paillier_sballot_test), in front of this.  The m_i and s_i are the voter's secrets: the staged words are overwritten here.
    Result<std::vector<AssignedBigUint<Fresh>>> sballot(Context& ctx, const EncryptionPublicKeyAssigned& pk_enc, const AssignedBigUint<Fresh>& hs,
                                                        const std::vector<AssignedWeight>& ms, const std::vector<AssignedBigUint<Fresh>>& ss,
                                                        unsigned m_bits) const {
        using R = Result<std::vector<AssignedBigUint<Fresh>>>;
        if (ms.empty() || ms.size() != ss.size() || ms.size() > 1024) return R::Err(PZ_ERR_INVALID, "sballot: one s per message, 1 .. 1024 of them");
        if (m_bits < 1 || m_bits > 64) return R::Err(PZ_ERR_INVALID, "sballot: m_bits outside 1 .. 64");
        const unsigned s_limbs = ss[0].num_limbs(), W = biguint->limb_bits;
        if (s_limbs < 1 || s_limbs > 2 * pk_enc.n.num_limbs()) return R::Err(PZ_ERR_INVALID, "sballot: an s of 1 .. 2 * n's limbs");
        if (hs.num_limbs() != 2 * pk_enc.n.num_limbs()) return R::Err(PZ_ERR_INVALID, "sballot: hs is not assigned at full width");
        auto n2m = biguint->square(ctx, pk_enc.n);
        if (!n2m.ok) return R::Err(n2m.err.status, n2m.err.msg);
        RefreshAux aux = RefreshAux::new_(W, pk_enc.n.num_limbs(), pk_enc.n.num_limbs());
        auto n2r = biguint->refresh(ctx, n2m.val, aux);
        if (!n2r.ok) return R::Err(n2r.err.status, n2r.err.msg);
        const AssignedBigUint<Fresh>& n2 = n2r.val;
        (void)ctx.load_zero();
        const unsigned L = n2.num_limbs(), Wd = n2.num_words(), wn = pk_enc.n.num_words(), wk = 2 * wn;   // K3 works on 2 * wn words
        const unsigned s_bits = s_limbs * W, sw = (s_bits + 63) / 64;
        std::vector<uint64_t> nv = pk_enc.n.words(), gv = pk_enc.g.value().to_limbs(wn), hv = hs.value().to_limbs(wk), mv, sv;
        for (const AssignedWeight& m : ms) mv.push_back(m.value);
        for (const auto& s : ss) {
            if (s.num_limbs() != s_limbs) return R::Err(PZ_ERR_INVALID, "sballot: the s_i are not assigned at one width");
            std::vector<uint64_t> w = s.value().to_limbs(sw);
            sv.insert(sv.end(), w.begin(), w.end());
        }
        const size_t K = ms.size(), per = 2 * (size_t)m_bits + 2 * (size_t)s_bits + 1;
        std::vector<uint64_t> rec(K * per * 4 * wk), cv(K * wk);
        int rc = pz_paillier_sballot(ctx.raw(), wn, K, m_bits, s_bits, nv.data(), gv.data(), hv.data(), mv.data(), sv.data(), rec.data(), K * per,
                                     cv.data());
        std::fill(mv.begin(), mv.end(), 0);
        std::fill(sv.begin(), sv.end(), 0);
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_paillier_sballot: ") + pz_strerror(rc));
        // the tape holds Wd words per integer (Wd < 2 * wn where limb_bits does not divide 64: the words above are zero)
        auto steps_of = [&](size_t at, std::vector<uint64_t>& out) {
            out.clear();
            for (size_t f = at * 4; f < (at + 1) * 4; ++f) {
                if (BigUint::from_limbs(rec.data() + f * wk, wk).bits() > (size_t)L * W) return false;
                out.insert(out.end(), rec.begin() + f * wk, rec.begin() + f * wk + Wd);
            }
            return true;
        };
        std::vector<uint64_t> steps;
        bool fits = true;
        auto bit_blocks = [&](size_t first, unsigned nbits) {   // nbits x (mul_mod, select, square_mod) from record `first` on
            for (unsigned j = 0; fits && j < nbits; ++j) {
                if (!(fits = steps_of(first + 2 * j, steps))) break;
                ctx.push_steps(steps, Wd, L, W, n2.value());
                ctx.record_cells(Context::SELECT, L, 8 * (size_t)L);
                if (!(fits = steps_of(first + 2 * j + 1, steps))) break;
                ctx.push_steps(steps, Wd, L, W, n2.value());
            }
        };
        std::vector<AssignedBigUint<Fresh>> out;
        for (size_t i = 0; fits && i < K; ++i) {
            (void)ctx.load_constant_one();
            (void)ctx.load_zero();
            ctx.record_cells(Context::NUM_TO_BITS, 1, 7 * (size_t)m_bits - 2);
            bit_blocks(i * per, m_bits);
            (void)ctx.load_constant_one();
            (void)ctx.load_zero();
            for (unsigned li = 0; fits && li < s_limbs; ++li) {
                ctx.record_cells(Context::NUM_TO_BITS, 1, 7 * (size_t)W - 2);
                bit_blocks(i * per + 2 * (size_t)m_bits + 2 * (size_t)li * W, W);
            }
            if (fits && (fits = steps_of((i + 1) * per - 1, steps))) ctx.push_steps(steps, Wd, L, W, n2.value());   // the final block
            out.push_back(AssignedBigUint<Fresh>(BigUint::from_limbs(cv.data() + i * wk, wk), L, W));
        }
        std::fill(rec.begin(), rec.end(), 0);
        if (!fits) return R::Err(PZ_ERR_RANGE, "a step's integer does not fit the assigned limb count");
        return R::Ok(out);
    }

    // The packed ballot: c_i = (prod_j G_j^v_ij) hs^s_i mod n^2 for R ciphertexts of K = gs.size() slots each
    // under one key and the public slot bases G_j = g^(2^(j w)) mod n^2 (pz::pballot_bases).  n^2 hoisted once, load_zero; per ciphertext,
    // per slot pow_mod(G_j, v_ij) over m_bits in-circuit bits as sballot's g-chain, then pow_mod(hs, s_i) as sballot, then the K fold
    // blocks.  One pz_paillier_pballot call computes every record; the tape takes them in the CIRCUIT's order -- slot chains, hs-chain,
    // folds -- which is the call's.  hs, the bases, the values' load_witness cells (vs[i][j]: ciphertext i, slot j), their sums and the
    // s_i are assigned by the caller (paillier_pballot_test), in front of this.  The v_ij and s_i are the voter's secrets: the staged
    // words are overwritten here.
    Result<std::vector<AssignedBigUint<Fresh>>> pballot(Context& ctx, const AssignedBigUint<Fresh>& n, const AssignedBigUint<Fresh>& hs,
                                                        const std::vector<AssignedBigUint<Fresh>>& gs,
                                                        const std::vector<std::vector<AssignedWeight>>& vs,
                                                        const std::vector<AssignedBigUint<Fresh>>& ss, unsigned m_bits) const {
        using R = Result<std::vector<AssignedBigUint<Fresh>>>;
        const size_t Rn = vs.size(), K = gs.size();
        if (Rn < 1 || Rn != ss.size() || Rn > 1024) return R::Err(PZ_ERR_INVALID, "pballot: one s per ciphertext, 1 .. 1024 of them");
        if (K < 1 || K > 64 || Rn * K > 1024) return R::Err(PZ_ERR_INVALID, "pballot: 1 .. 64 slots, at most 1024 values in all");
        if (m_bits < 1 || m_bits > 64) return R::Err(PZ_ERR_INVALID, "pballot: m_bits outside 1 .. 64");
        const unsigned s_limbs = ss[0].num_limbs(), W = biguint->limb_bits;
        if (s_limbs < 1 || s_limbs > 2 * n.num_limbs()) return R::Err(PZ_ERR_INVALID, "pballot: an s of 1 .. 2 * n's limbs");
        if (hs.num_limbs() != 2 * n.num_limbs()) return R::Err(PZ_ERR_INVALID, "pballot: hs is not assigned at full width");
        for (const auto& gj : gs)
            if (gj.num_limbs() != 2 * n.num_limbs()) return R::Err(PZ_ERR_INVALID, "pballot: a slot base is not assigned at full width");
        for (const auto& row : vs)
            if (row.size() != K) return R::Err(PZ_ERR_INVALID, "pballot: one value per slot in every ciphertext");
        auto n2m = biguint->square(ctx, n);
        if (!n2m.ok) return R::Err(n2m.err.status, n2m.err.msg);
        RefreshAux aux = RefreshAux::new_(W, n.num_limbs(), n.num_limbs());
        auto n2r = biguint->refresh(ctx, n2m.val, aux);
        if (!n2r.ok) return R::Err(n2r.err.status, n2r.err.msg);
        const AssignedBigUint<Fresh>& n2 = n2r.val;
        (void)ctx.load_zero();
        const unsigned L = n2.num_limbs(), Wd = n2.num_words(), wn = n.num_words(), wk = 2 * wn;   // K3 works on 2 * wn words
        const unsigned s_bits = s_limbs * W, sw = (s_bits + 63) / 64;
        std::vector<uint64_t> nv = n.words(), hv = hs.value().to_limbs(wk), gv, vv, sv;
        for (const auto& gj : gs) {
            std::vector<uint64_t> w = gj.value().to_limbs(wk);
            gv.insert(gv.end(), w.begin(), w.end());
        }
        for (const auto& row : vs)
            for (const AssignedWeight& v : row) vv.push_back(v.value);
        for (const auto& s : ss) {
            if (s.num_limbs() != s_limbs) return R::Err(PZ_ERR_INVALID, "pballot: the s_i are not assigned at one width");
            std::vector<uint64_t> w = s.value().to_limbs(sw);
            sv.insert(sv.end(), w.begin(), w.end());
        }
        const size_t per = 2 * (size_t)m_bits * K + 2 * (size_t)s_bits + K;
        std::vector<uint64_t> rec(Rn * per * 4 * wk), cv(Rn * wk);
        int rc = pz_paillier_pballot(ctx.raw(), wn, Rn, (uint32_t)K, m_bits, s_bits, nv.data(), hv.data(), gv.data(), vv.data(), sv.data(),
                                     rec.data(), Rn * per, cv.data());
        std::fill(vv.begin(), vv.end(), 0);
        std::fill(sv.begin(), sv.end(), 0);
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_paillier_pballot: ") + pz_strerror(rc));
        // the tape holds Wd words per integer (Wd < 2 * wn where limb_bits does not divide 64: the words above are zero)
        auto steps_of = [&](size_t at, std::vector<uint64_t>& out) {
            out.clear();
            for (size_t f = at * 4; f < (at + 1) * 4; ++f) {
                if (BigUint::from_limbs(rec.data() + f * wk, wk).bits() > (size_t)L * W) return false;
                out.insert(out.end(), rec.begin() + f * wk, rec.begin() + f * wk + Wd);
            }
            return true;
        };
        std::vector<uint64_t> steps;
        bool fits = true;
        auto bit_blocks = [&](size_t first, unsigned nbits) {   // nbits x (mul_mod, select, square_mod) from record `first` on
            for (unsigned j = 0; fits && j < nbits; ++j) {
                if (!(fits = steps_of(first + 2 * j, steps))) break;
                ctx.push_steps(steps, Wd, L, W, n2.value());
                ctx.record_cells(Context::SELECT, L, 8 * (size_t)L);
                if (!(fits = steps_of(first + 2 * j + 1, steps))) break;
                ctx.push_steps(steps, Wd, L, W, n2.value());
            }
        };
        std::vector<AssignedBigUint<Fresh>> out;
        for (size_t i = 0; fits && i < Rn; ++i) {
            for (size_t j = 0; fits && j < K; ++j) {
                (void)ctx.load_constant_one();
                (void)ctx.load_zero();
                ctx.record_cells(Context::NUM_TO_BITS, 1, 7 * (size_t)m_bits - 2);
                bit_blocks(i * per + 2 * (size_t)m_bits * j, m_bits);
            }
            (void)ctx.load_constant_one();
            (void)ctx.load_zero();
            for (unsigned li = 0; fits && li < s_limbs; ++li) {
                ctx.record_cells(Context::NUM_TO_BITS, 1, 7 * (size_t)W - 2);
                bit_blocks(i * per + 2 * (size_t)m_bits * K + 2 * (size_t)li * W, W);
            }
            for (size_t q = 0; fits && q < K; ++q)   // the folds
                if ((fits = steps_of((i + 1) * per - K + q, steps))) ctx.push_steps(steps, Wd, L, W, n2.value());
            out.push_back(AssignedBigUint<Fresh>(BigUint::from_limbs(cv.data() + i * wk, wk), L, W));
        }
        std::fill(rec.begin(), rec.end(), 0);
        if (!fits) return R::Err(PZ_ERR_RANGE, "a step's integer does not fit the assigned limb count");
        return R::Ok(out);
    }

    // The mix: c'_i = c_perm(i) r_i^n mod n^2 for K = 2^d ciphertexts under one key -- perm[i] is the index of
    // the input that output i receives.  n^2 hoisted once, load_zero; the Benes network switch by switch (benes_route gives the bits);
    // per output pow_mod_fixed_exp(r_i_ext, n) and mul_mod(d_i, rn_i).  One pz_paillier_mix call computes every route layer and record;
    // the tape takes the records in the circuit's order, which is the call's.  The ciphertexts and the r_i are assigned by the caller
    // (paillier_mix_test), in front of this.  wit (may be null) keeps the bits and the route layers, which the expansion of the tape
    // needs (synthesize_mix_circuit) and which are the mixer's secrets: the caller wipes them.
    struct MixWitness {
        std::vector<uint8_t> bits;        // (2d - 1) K / 2 switch bytes, layer-major
        std::vector<uint64_t> routes;     // (2d - 1) x K x 2 wn words: every layer's outputs, as pz_paillier_mix leaves them
        void wipe() {
            std::fill(bits.begin(), bits.end(), 0);
            std::fill(routes.begin(), routes.end(), 0);
        }
    };
    Result<std::vector<AssignedBigUint<Fresh>>> mix(Context& ctx, const AssignedBigUint<Fresh>& n, const std::vector<AssignedBigUint<Fresh>>& cts,
                                                    const std::vector<uint32_t>& perm, const std::vector<AssignedBigUint<Fresh>>& rs,
                                                    MixWitness* wit) const {
        using R = Result<std::vector<AssignedBigUint<Fresh>>>;
        const size_t K = cts.size();
        if (!benes_is_count(K) || rs.size() != K || perm.size() != K) return R::Err(PZ_ERR_INVALID, "mix: 1, 2, 4 .. 1024 ciphertexts, one r and one index each");
        std::vector<uint8_t> bits;
        if (!benes_route(K, perm.data(), bits)) return R::Err(PZ_ERR_INVALID, "mix: perm is no permutation of 0 .. K - 1");
        auto n2m = biguint->square(ctx, n);
        if (!n2m.ok) return R::Err(n2m.err.status, n2m.err.msg);
        RefreshAux aux = RefreshAux::new_(biguint->limb_bits, n.num_limbs(), n.num_limbs());
        auto n2r = biguint->refresh(ctx, n2m.val, aux);
        if (!n2r.ok) return R::Err(n2r.err.status, n2r.err.msg);
        const AssignedBigUint<Fresh>& n2 = n2r.val;
        (void)ctx.load_zero();
        const unsigned L = n2.num_limbs(), Wd = n2.num_words(), wn = n.num_words(), wk = 2 * wn;   // K3 works on 2 * wn words
        std::vector<uint64_t> nv = n.words(), cv, rv;
        for (const auto& c : cts) {
            if (c.num_limbs() != L) return R::Err(PZ_ERR_INVALID, "mix: a ciphertext is not assigned at full width");
            std::vector<uint64_t> w = c.value().to_limbs(wk);
            cv.insert(cv.end(), w.begin(), w.end());
        }
        for (const auto& r : rs) {
            if (r.num_limbs() != n.num_limbs()) return R::Err(PZ_ERR_INVALID, "mix: an r is not assigned at n's width");
            std::vector<uint64_t> w = r.value().to_limbs(wn);
            rv.insert(rv.end(), w.begin(), w.end());
        }
        size_t nr = n.value().bits();
        for (uint64_t w : nv) nr += (size_t)__builtin_popcountll(w);
        const size_t per = nr + 1, layers = benes_layers(K);
        std::vector<uint64_t> routes(layers * K * wk + 1), rec(K * per * 4 * wk), mv(K * wk);
        int rc = pz_paillier_mix(ctx.raw(), wn, K, nv.data(), cv.data(), bits.data(), rv.data(), routes.data(), rec.data(), K * per, mv.data());
        std::fill(rv.begin(), rv.end(), 0);
        auto fail = [&](int st, const std::string& m) {
            std::fill(bits.begin(), bits.end(), 0);
            std::fill(routes.begin(), routes.end(), 0);
            std::fill(rec.begin(), rec.end(), 0);
            return R::Err(st, m);
        };
        if (rc != PZ_OK) return fail(rc, std::string("pz_paillier_mix: ") + pz_strerror(rc));
        for (size_t s = 0; s < layers * (K / 2); ++s) ctx.conditional_swap(L);
        // the tape holds Wd words per integer (Wd < 2 * wn where limb_bits does not divide 64: the words above are zero)
        std::vector<uint64_t> steps;
        std::vector<AssignedBigUint<Fresh>> out;
        for (size_t i = 0; i < K; ++i) {
            (void)ctx.load_constant_one();
            (void)ctx.load_zero();
            steps.clear();
            for (size_t f = i * per * 4; f < (i + 1) * per * 4; ++f) {
                if (BigUint::from_limbs(rec.data() + f * wk, wk).bits() > (size_t)L * biguint->limb_bits)
                    return fail(PZ_ERR_RANGE, "a step's integer does not fit the assigned limb count");
                steps.insert(steps.end(), rec.begin() + f * wk, rec.begin() + f * wk + Wd);
            }
            ctx.push_steps(steps, Wd, L, biguint->limb_bits, n2.value());   // the r^n chain, then the final block
            out.push_back(AssignedBigUint<Fresh>(BigUint::from_limbs(mv.data() + i * wk, wk), L, biguint->limb_bits));
        }
        std::fill(rec.begin(), rec.end(), 0);
        std::fill(steps.begin(), steps.end(), 0);
        routes.resize(layers * K * wk);
        if (wit) {
            wit->bits = bits;
            wit->routes = routes;
        }
        std::fill(bits.begin(), bits.end(), 0);
        std::fill(routes.begin(), routes.end(), 0);
        return R::Ok(out);
    }

    // The short-randomness mix: c'_i = c_perm(i) hs^s_i mod n^2 for K = 2^d ciphertexts under one key (n, hs)
    // -- mix with every r_i^n chain replaced by sballot's hs-chain.  n^2 hoisted once, load_zero; the Benes network switch by switch;
    // per output [1, 0], per limb of s_i num_to_bits and that limb's blocks, and mul_mod(d_i, hss_i).  One pz_paillier_smix call
    // computes every route layer and record; the tape takes the records in the circuit's order, which is the call's.  hs, the
    // ciphertexts and the s_i (all of ONE limb count, 1 .. 2 * n's) are assigned by the caller (paillier_smix_test), in front of this.
    // wit (may be null) keeps the bits and the route layers for synthesize_smix_circuit: the mixer's secrets, which the caller wipes.
    Result<std::vector<AssignedBigUint<Fresh>>> smix(Context& ctx, const AssignedBigUint<Fresh>& n, const AssignedBigUint<Fresh>& hs,
                                                     const std::vector<AssignedBigUint<Fresh>>& cts, const std::vector<uint32_t>& perm,
                                                     const std::vector<AssignedBigUint<Fresh>>& ss, MixWitness* wit) const {
        using R = Result<std::vector<AssignedBigUint<Fresh>>>;
        const size_t K = cts.size();
        if (!benes_is_count(K) || ss.size() != K || perm.size() != K) return R::Err(PZ_ERR_INVALID, "smix: 1, 2, 4 .. 1024 ciphertexts, one s and one index each");
        const unsigned s_limbs = ss[0].num_limbs(), W = biguint->limb_bits;
        if (s_limbs < 1 || s_limbs > 2 * n.num_limbs()) return R::Err(PZ_ERR_INVALID, "smix: an s of 1 .. 2 * n's limbs");
        if (hs.num_limbs() != 2 * n.num_limbs()) return R::Err(PZ_ERR_INVALID, "smix: hs is not assigned at full width");
        std::vector<uint8_t> bits;
        if (!benes_route(K, perm.data(), bits)) return R::Err(PZ_ERR_INVALID, "smix: perm is no permutation of 0 .. K - 1");
        auto n2m = biguint->square(ctx, n);
        if (!n2m.ok) return R::Err(n2m.err.status, n2m.err.msg);
        RefreshAux aux = RefreshAux::new_(W, n.num_limbs(), n.num_limbs());
        auto n2r = biguint->refresh(ctx, n2m.val, aux);
        if (!n2r.ok) return R::Err(n2r.err.status, n2r.err.msg);
        const AssignedBigUint<Fresh>& n2 = n2r.val;
        (void)ctx.load_zero();
        const unsigned L = n2.num_limbs(), Wd = n2.num_words(), wn = n.num_words(), wk = 2 * wn;   // K3 works on 2 * wn words
        const unsigned s_bits = s_limbs * W, sw = (s_bits + 63) / 64;
        std::vector<uint64_t> nv = n.words(), hv = hs.value().to_limbs(wk), cv, sv;
        for (const auto& c : cts) {
            if (c.num_limbs() != L) return R::Err(PZ_ERR_INVALID, "smix: a ciphertext is not assigned at full width");
            std::vector<uint64_t> w = c.value().to_limbs(wk);
            cv.insert(cv.end(), w.begin(), w.end());
        }
        for (const auto& x : ss) {
            if (x.num_limbs() != s_limbs) {
                std::fill(sv.begin(), sv.end(), 0);
                return R::Err(PZ_ERR_INVALID, "smix: the s_i are not assigned at one width");
            }
            std::vector<uint64_t> w = x.value().to_limbs(sw);
            sv.insert(sv.end(), w.begin(), w.end());
        }
        const size_t per = 2 * (size_t)s_bits + 1, layers = benes_layers(K);
        std::vector<uint64_t> routes(layers * K * wk + 1), rec(K * per * 4 * wk), mv(K * wk);
        int rc = pz_paillier_smix(ctx.raw(), wn, K, s_bits, nv.data(), hv.data(), cv.data(), bits.data(), sv.data(), routes.data(), rec.data(), K * per,
                                  mv.data());
        std::fill(sv.begin(), sv.end(), 0);
        auto fail = [&](int st, const std::string& m) {
            std::fill(bits.begin(), bits.end(), 0);
            std::fill(routes.begin(), routes.end(), 0);
            std::fill(rec.begin(), rec.end(), 0);
            return R::Err(st, m);
        };
        if (rc != PZ_OK) return fail(rc, std::string("pz_paillier_smix: ") + pz_strerror(rc));
        for (size_t s = 0; s < layers * (K / 2); ++s) ctx.conditional_swap(L);
        // the tape holds Wd words per integer (Wd < 2 * wn where limb_bits does not divide 64: the words above are zero)
        std::vector<uint64_t> steps;
        auto steps_of = [&](size_t at) {
            steps.clear();
            for (size_t f = at * 4; f < (at + 1) * 4; ++f) {
                if (BigUint::from_limbs(rec.data() + f * wk, wk).bits() > (size_t)L * W) return false;
                steps.insert(steps.end(), rec.begin() + f * wk, rec.begin() + f * wk + Wd);
            }
            return true;
        };
        std::vector<AssignedBigUint<Fresh>> out;
        bool fits = true;
        for (size_t i = 0; fits && i < K; ++i) {
            (void)ctx.load_constant_one();
            (void)ctx.load_zero();
            for (unsigned li = 0; fits && li < s_limbs; ++li) {
                ctx.record_cells(Context::NUM_TO_BITS, 1, 7 * (size_t)W - 2);
                for (unsigned j = 0; fits && j < W; ++j) {   // W x (mul_mod, select, square_mod)
                    const size_t first = i * per + 2 * ((size_t)li * W + j);
                    if (!(fits = steps_of(first))) break;
                    ctx.push_steps(steps, Wd, L, W, n2.value());
                    ctx.record_cells(Context::SELECT, L, 8 * (size_t)L);
                    if (!(fits = steps_of(first + 1))) break;
                    ctx.push_steps(steps, Wd, L, W, n2.value());
                }
            }
            if (fits && (fits = steps_of((i + 1) * per - 1))) ctx.push_steps(steps, Wd, L, W, n2.value());   // the final block
            out.push_back(AssignedBigUint<Fresh>(BigUint::from_limbs(mv.data() + i * wk, wk), L, W));
        }
        std::fill(steps.begin(), steps.end(), 0);
        if (!fits) return fail(PZ_ERR_RANGE, "a step's integer does not fit the assigned limb count");
        std::fill(rec.begin(), rec.end(), 0);
        routes.resize(layers * K * wk);
        if (wit) {
            wit->bits = bits;
            wit->routes = routes;
        }
        std::fill(bits.begin(), bits.end(), 0);
        std::fill(routes.begin(), routes.end(), 0);
        return R::Ok(out);
    }

    // Decryption with randomness recovery, the key holder's step after `tally`: one pz_paillier_decrypt call
    // over all ciphertexts.  Nothing goes on the tape: the proof that c decrypts to m is the uniform-shape circuit run on the (m, r)
    // returned here, under the statement n | g | m | c (circuit kind 5).
    // crt: CrtPath::No the lambda path, Yes the CRT path (PZ_ERR_INVALID on a handle without one), Auto the CRT path where the handle
    // has one and the shape is one at which it is no slower (section 15.22); the results are the same bit for bit.
    Result<std::vector<Decryption>> decrypt(Context& ctx, const PaillierSecretKey& sk, const std::vector<BigUint>& cts, bool want_r = true,
                                            CrtPath crt = CrtPath::Auto) const {
        using R = Result<std::vector<Decryption>>;
        // Auto: where the probe found the CRT path no slower (profiles/decrypt_crt_probe.jsonl) -- n^2 beyond the 64-limb instantiation, or
        // the 2 B half-length teams resident at once (256 CUs x 2 teams)
        const bool use_crt = crt == CrtPath::Yes || (crt == CrtPath::Auto && sk.has_crt() && (sk.words() > 32 || 2 * cts.size() <= 512));
        const unsigned Ln = sk.words();
        std::vector<uint64_t> cv;
        for (const BigUint& c : cts) {
            if (c.l.size() > 2 * (size_t)Ln) return R::Err(PZ_ERR_RANGE, "decrypt: a ciphertext is wider than n^2");
            std::vector<uint64_t> w = c.to_limbs(2 * Ln);
            cv.insert(cv.end(), w.begin(), w.end());
        }
        std::vector<uint64_t> m(cts.size() * Ln), r(want_r ? cts.size() * Ln : 0);
        std::vector<uint8_t> flags(cts.size());
        int rc = (use_crt ? pz_paillier_decrypt_crt : pz_paillier_decrypt)(ctx.raw(), sk.raw(), cts.size(), cv.data(), m.data(),
                                                                           want_r ? r.data() : nullptr, flags.data());
        if (rc != PZ_OK) return R::Err(rc, std::string(use_crt ? "pz_paillier_decrypt_crt: " : "pz_paillier_decrypt: ") + pz_strerror(rc));
        std::vector<Decryption> out(cts.size());
        for (size_t i = 0; i < cts.size(); ++i) {
            out[i].m = BigUint::from_limbs(m.data() + i * Ln, Ln);
            if (want_r) out[i].r = BigUint::from_limbs(r.data() + i * Ln, Ln);
            out[i].unit = flags[i] == 0;
        }
        return R::Ok(out);
    }

    // A trustee's partial decryptions: h = v^theta and u_j = (c_j^2)^theta mod n^2 over the circuit's own
    // 2 * enc_bits exponent bits, one pz_paillier_partial call for all ciphertexts.  Nothing goes on the tape: the proof is circuit kind 7
    // run on the records of pz_paillier_partial_dev.  theta is the trustee's secret: the staged words are overwritten here too.
    Result<PartialDecryption> partial_decrypt(Context& ctx, const BigUint& n, const BigUint& v, const BigUint& theta,
                                              const std::vector<BigUint>& cts) const {
        using R = Result<PartialDecryption>;
        const size_t Ln = std::max<size_t>(1, n.l.size()), L = 2 * Ln;
        if (cts.empty() || cts.size() > 1024) return R::Err(PZ_ERR_INVALID, "partial_decrypt: 1 .. 1024 ciphertexts");
        if (2 * (size_t)enc_bits > 128 * Ln) return R::Err(PZ_ERR_INVALID, "partial_decrypt: enc_bits is wider than n's words");
        if (v.l.size() > L || theta.l.size() > L) return R::Err(PZ_ERR_RANGE, "partial_decrypt: v or theta is wider than n^2");
        std::vector<uint64_t> cv;
        for (const BigUint& c : cts) {
            if (c.l.size() > L) return R::Err(PZ_ERR_RANGE, "partial_decrypt: a ciphertext is wider than n^2");
            std::vector<uint64_t> w = c.to_limbs(L);
            cv.insert(cv.end(), w.begin(), w.end());
        }
        std::vector<uint64_t> nv = n.to_limbs(Ln), vv = v.to_limbs(L), tv = theta.to_limbs(L), h(L), u(cts.size() * L);
        int rc = pz_paillier_partial(ctx.raw(), (uint32_t)Ln, cts.size(), 2 * enc_bits, nv.data(), vv.data(), tv.data(), cv.data(), nullptr, 0,
                                     h.data(), u.data());
        std::fill(tv.begin(), tv.end(), 0);
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_paillier_partial: ") + pz_strerror(rc));
        PartialDecryption out;
        out.h = BigUint::from_limbs(h.data(), L);
        for (size_t j = 0; j < cts.size(); ++j) out.us.push_back(BigUint::from_limbs(u.data() + j * L, L));
        return R::Ok(out);
    }

    // The combiner: m_j = L(prod_i u_ij mod n^2) mu2 mod n over the T trustees' partials (partials[i] = trustee i's us), one
    // pz_paillier_combine call.  `unit` is false (and m zero) where the product is not 1 mod n: the partials do not belong together.
    Result<std::vector<Decryption>> combine(Context& ctx, const ThresholdKey& key, const std::vector<std::vector<BigUint>>& partials) const {
        using R = Result<std::vector<Decryption>>;
        const size_t Ln = std::max<size_t>(1, key.n.l.size()), L = 2 * Ln, T = partials.size(), K = T ? partials[0].size() : 0;
        if (T < 1 || T > 256 || K < 1 || K > 1024) return R::Err(PZ_ERR_INVALID, "combine: 1 .. 256 trustees, 1 .. 1024 ciphertexts");
        if (key.mu2.l.size() > Ln) return R::Err(PZ_ERR_RANGE, "combine: mu2 is wider than n");
        std::vector<uint64_t> pv;
        for (const auto& row : partials) {
            if (row.size() != K) return R::Err(PZ_ERR_INVALID, "combine: every trustee answers every ciphertext");
            for (const BigUint& u : row) {
                if (u.l.size() > L) return R::Err(PZ_ERR_RANGE, "combine: a partial is wider than n^2");
                std::vector<uint64_t> w = u.to_limbs(L);
                pv.insert(pv.end(), w.begin(), w.end());
            }
        }
        std::vector<uint64_t> nv = key.n.to_limbs(Ln), mv = key.mu2.to_limbs(Ln), m(K * Ln);
        std::vector<uint8_t> flags(K);
        int rc = pz_paillier_combine(ctx.raw(), (uint32_t)Ln, K, T, nv.data(), mv.data(), pv.data(), m.data(), flags.data());
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_paillier_combine: ") + pz_strerror(rc));
        std::vector<Decryption> out(K);
        for (size_t j = 0; j < K; ++j) {
            out[j].m = BigUint::from_limbs(m.data() + j * Ln, Ln);
            out[j].unit = flags[j] == 0;
        }
        return R::Ok(out);
    }

    // The t-of-T combiner: the members `ids` (distinct trustee ids, 1-based; any key.threshold of them) answer
    // with partials[k] = member ids[k]'s us; the Lagrange exponents come from pz_shamir_lagrange, the plaintexts from one
    // pz_paillier_combine_t call.  `unit` is false (and m zero) where the partials do not belong together, are too few, or B mod n is no unit.
    Result<std::vector<Decryption>> combine_t(Context& ctx, const ShamirKey& key, const std::vector<uint32_t>& ids,
                                              const std::vector<std::vector<BigUint>>& partials) const {
        using R = Result<std::vector<Decryption>>;
        const size_t Ln = std::max<size_t>(1, key.n.l.size()), L = 2 * Ln, M = partials.size(), K = M ? partials[0].size() : 0;
        if (M < 1 || M > 256 || M != ids.size() || K < 1 || K > 1024)
            return R::Err(PZ_ERR_INVALID, "combine_t: 1 .. 256 members with an id each, 1 .. 1024 ciphertexts");
        if (key.mu2.l.size() > Ln) return R::Err(PZ_ERR_RANGE, "combine_t: mu2 is wider than n");
        const uint32_t cap = 64;
        std::vector<uint64_t> exps(M * cap);
        std::vector<uint8_t> neg(M);
        int rc = pz_shamir_lagrange((uint32_t)key.trustees, M, ids.data(), exps.data(), cap, neg.data(), nullptr);
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_shamir_lagrange: ") + pz_strerror(rc));
        std::vector<uint64_t> pv;
        for (const auto& row : partials) {
            if (row.size() != K) return R::Err(PZ_ERR_INVALID, "combine_t: every member answers every ciphertext");
            for (const BigUint& u : row) {
                if (u.l.size() > L) return R::Err(PZ_ERR_RANGE, "combine_t: a partial is wider than n^2");
                std::vector<uint64_t> w = u.to_limbs(L);
                pv.insert(pv.end(), w.begin(), w.end());
            }
        }
        std::vector<uint64_t> nv = key.n.to_limbs(Ln), mv = key.mu2.to_limbs(Ln), m(K * Ln);
        std::vector<uint8_t> flags(K);
        rc = pz_paillier_combine_t(ctx.raw(), (uint32_t)Ln, K, M, nv.data(), mv.data(), exps.data(), cap, neg.data(), pv.data(), m.data(),
                                   flags.data());
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_paillier_combine_t: ") + pz_strerror(rc));
        std::vector<Decryption> out(K);
        for (size_t j = 0; j < K; ++j) {
            out[j].m = BigUint::from_limbs(m.data() + j * Ln, Ln);
            out[j].unit = flags[j] == 0;
        }
        return R::Ok(out);
    }

    // x^-1 mod `mod` for a batch under one odd modulus, one pz_bigint_mod_inverse call; an x without an inverse (zero included) comes
    // back as zero, which is no value's inverse.  An x >= mod is PZ_ERR_RANGE.
    Result<std::vector<BigUint>> mod_inverse(Context& ctx, const BigUint& mod, const std::vector<BigUint>& xs) const {
        using R = Result<std::vector<BigUint>>;
        const size_t L = std::max<size_t>(1, mod.l.size());
        if (xs.empty() || xs.size() > 65536) return R::Err(PZ_ERR_INVALID, "mod_inverse: 1 .. 65536 values");
        std::vector<uint64_t> xv;
        for (const BigUint& x : xs) {
            if (x.l.size() > L) return R::Err(PZ_ERR_RANGE, "mod_inverse: a value is wider than the modulus");
            std::vector<uint64_t> w = x.to_limbs(L);
            xv.insert(xv.end(), w.begin(), w.end());
        }
        std::vector<uint64_t> mv = mod.to_limbs(L), inv(xs.size() * L);
        std::vector<uint8_t> flags(xs.size());
        int rc = pz_bigint_mod_inverse(ctx.raw(), (uint32_t)L, xs.size(), mv.data(), xv.data(), inv.data(), flags.data());
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_bigint_mod_inverse: ") + pz_strerror(rc));
        std::vector<BigUint> out;
        for (size_t j = 0; j < xs.size(); ++j) out.push_back(BigUint::from_limbs(inv.data() + j * L, L));
        return R::Ok(out);
    }

    // Miller-Rabin on the device, every value its own modulus (pz_bigint_is_prime): true where x passes every
    // round over `bases` (1 .. 64 words, each >= 2).  Values of up to 2048 bits; a wider one is PZ_ERR_RANGE.
    Result<std::vector<bool>> is_probable_prime(Context& ctx, const std::vector<BigUint>& xs, const std::vector<uint64_t>& bases) const {
        using R = Result<std::vector<bool>>;
        if (xs.empty() || xs.size() > 65536) return R::Err(PZ_ERR_INVALID, "is_probable_prime: 1 .. 65536 values");
        size_t L = 1;
        for (const BigUint& x : xs) L = std::max(L, x.l.size());
        if (L > 32) return R::Err(PZ_ERR_RANGE, "is_probable_prime: a value is wider than 2048 bits");
        std::vector<uint64_t> xv;
        for (const BigUint& x : xs) {
            std::vector<uint64_t> w = x.to_limbs(L);
            xv.insert(xv.end(), w.begin(), w.end());
        }
        std::vector<uint8_t> flags(xs.size());
        std::vector<uint32_t> witness(xs.size());
        int rc = pz_bigint_is_prime(ctx.raw(), (uint32_t)L, xs.size(), xv.data(), (uint32_t)bases.size(), bases.data(), flags.data(), witness.data());
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_bigint_is_prime: ") + pz_strerror(rc));
        return R::Ok(std::vector<bool>(flags.begin(), flags.end()));
    }
    // the `want` smallest offsets i of the window start + stride i (stride 2; 4 with safe) that survive the sieve and every round -- with
    // safe, whose (c - 1) / 2 passes too (pz_prime_search).  Fewer than want, or none, is Ok.
    Result<std::vector<uint32_t>> prime_search(Context& ctx, const BigUint& start, size_t limbs, size_t window, bool safe,
                                               const std::vector<uint64_t>& bases, uint32_t want) const {
        using R = Result<std::vector<uint32_t>>;
        if (limbs < 1 || limbs > 32 || start.l.size() > limbs) return R::Err(PZ_ERR_RANGE, "prime_search: the start does not fit 1 .. 32 words");
        if (want < 1 || want > 64) return R::Err(PZ_ERR_INVALID, "prime_search: want outside 1 .. 64");
        std::vector<uint64_t> sv = start.to_limbs(limbs);
        std::vector<uint32_t> offs(want);
        uint32_t found = 0;
        int rc = pz_prime_search(ctx.raw(), (uint32_t)limbs, sv.data(), window, safe ? 1 : 0, (uint32_t)bases.size(), bases.data(), want, offs.data(),
                                 &found, nullptr);
        if (rc != PZ_OK) return R::Err(rc, std::string("pz_prime_search: ") + pz_strerror(rc));
        offs.resize(found);
        return R::Ok(offs);
    }

    // c^w mod n^2 = Enc(w m): the weighted tally of one ciphertext
    Result<AssignedBigUint<Fresh>> mul_scalar(Context& ctx, const EncryptionPublicKeyAssigned& pk_enc, const AssignedBigUint<Fresh>& c,
                                              const AssignedWeight& w, unsigned w_bits) const {
        return weighted_tally(ctx, pk_enc, {c}, {w}, w_bits);
    }
};

// The dealer of a T-of-T threshold key (keys.py::deal_shares is the same in Python integers): theta = lambda
// (lambda^-1 mod n), theta_1 .. theta_{T-1} = rand(n lambda), theta_T = (theta - their sum) mod n lambda; v = w^2 mod n^2 for a drawn w;
// h_i = v^theta_i and g^theta through PaillierChip::partial_decrypt (the device's chains), mu2 = (2a)^-1 mod n.  rand(k): uniform in
// [0, k), from the caller's CSPRNG.  safe_primes: the caller's word that (p - 1) / 2 and (q - 1) / 2 are prime (pz::primes_are_safe derives it on
// the device): v is then resampled until v^(N/2) = 1 and v^((N/2)/l) != 1 for l in {p, q, (p - 1) / 2, (q - 1) / 2}, N = n lambda,
// and the key says v_order_proved.  Refuses p = q, even or tiny primes, gcd(n, phi(n)) != 1, a g whose order n does not divide, and
// trustees outside 1 .. 256 (PZ_ERR_INVALID).  The dealer forgets p, q, lambda, theta and the shares it hands out.
inline BigUint paillier_add_native(Context& ctx, const BigUint& n, const BigUint& c1, const BigUint& c2);
struct DealtShares {
    ThresholdKey key;
    std::vector<BigUint> shares;
};
inline Result<DealtShares> deal_shares(Context& ctx, const PaillierChip& chip, const BigUint& p, const BigUint& q, size_t trustees,
                                       const std::function<BigUint(const BigUint&)>& rand, bool safe_primes = false,
                                       const BigUint* g_in = nullptr) {
    using R = Result<DealtShares>;
    const BigUint one(1), two(2);
    if (trustees < 1 || trustees > 256) return R::Err(PZ_ERR_INVALID, "deal_shares: trustees outside 1 .. 256");
    if (p < BigUint(3) || q < BigUint(3) || p == q || !p.bit(0) || !q.bit(0)) return R::Err(PZ_ERR_INVALID, "deal_shares: p and q must be distinct odd primes");
    const BigUint n = p * q, n2 = n * n, p1 = p - one, q1 = q - one;
    if (BigUint::gcd(n, p1 * q1) != one) return R::Err(PZ_ERR_INVALID, "deal_shares: gcd(n, phi(n)) != 1");
    const BigUint lambda = (p1 * q1) / BigUint::gcd(p1, q1), N = n * lambda, theta = lambda * BigUint::mod_inverse(lambda, n);
    DealtShares out;
    out.key.n = n;
    out.key.g = g_in ? *g_in : n + one;
    if (out.key.g.is_zero() || !(out.key.g < n2)) return R::Err(PZ_ERR_INVALID, "deal_shares: g outside (0, n^2)");
    const std::vector<BigUint> unit{one};
    auto power = [&](const BigUint& base, const BigUint& e) { return chip.partial_decrypt(ctx, n, base, e, unit); };   // base^e mod n^2
    // 1 + a n = g^theta mod n^2 with a a unit mod n: n divides the order of g
    auto gt = power(out.key.g, theta);
    if (!gt.ok) return R::Err(gt.err.status, gt.err.msg);
    BigUint a, rem;
    BigUint::divmod(gt.val.h, n, a, rem);
    if (rem != one || BigUint::gcd(a % n, n) != one) return R::Err(PZ_ERR_INVALID, "deal_shares: n does not divide the order of g");
    out.key.mu2 = BigUint::mod_inverse((two * a) % n, n);
    BigUint sum;
    for (size_t i = 0; i + 1 < trustees; ++i) {
        out.shares.push_back(rand(N) % N);
        sum = (sum + out.shares.back()) % N;
    }
    out.shares.push_back((theta + N - sum) % N);
    const BigUint pp = p1 / two, qq = q1 / two, half = N / two;
    for (;;) {
        const BigUint w = rand(n2) % n2;
        if (w < two || BigUint::gcd(w, n) != one) continue;
        const BigUint v = paillier_add_native(ctx, n, w, w);   // w^2 mod n^2
        if (v == one) continue;
        bool good = true;
        if (safe_primes) {
            auto full = power(v, half);
            if (!full.ok) return R::Err(full.err.status, full.err.msg);
            good = full.val.h == one;
            for (const BigUint* l : {&p, &q, &pp, &qq}) {
                if (!good) break;
                auto part = power(v, half / *l);
                if (!part.ok) return R::Err(part.err.status, part.err.msg);
                good = part.val.h != one;
            }
        }
        if (good) {
            out.key.v = v;
            break;
        }
    }
    out.key.v_order_proved = safe_primes;
    for (const BigUint& s : out.shares) {
        auto h = power(out.key.v, s);
        if (!h.ok) return R::Err(h.err.status, h.err.msg);
        out.key.hs.push_back(h.val.h);
    }
    return R::Ok(out);
}

// The dealer of a t-of-T key (keys.py::deal_shamir is the same in Python integers): a_1 .. a_{t-1} =
// rand(n lambda), f(X) = theta + sum a_k X^k, s_i = f(i) mod n lambda by Horner's rule on the host; v chosen and, on the caller's word
// about safe primes, order-checked exactly as deal_shares does; h_i = v^(s_i) and g^theta from the device's chains; mu2 =
// (2 a trustees!)^-1 mod n.  Refuses what deal_shares refuses, a threshold outside 1 .. trustees and primes that do not exceed the
// number of trustees (trustees! must be a unit mod n): PZ_ERR_INVALID.  The dealer forgets p, q, lambda, theta, f and the shares.
struct DealtShamir {
    ShamirKey key;
    std::vector<BigUint> shares;
};
inline Result<DealtShamir> deal_shamir(Context& ctx, const PaillierChip& chip, const BigUint& p, const BigUint& q, size_t trustees,
                                       size_t threshold, const std::function<BigUint(const BigUint&)>& rand, bool safe_primes = false,
                                       const BigUint* g_in = nullptr) {
    using R = Result<DealtShamir>;
    const BigUint one(1), two(2);
    if (trustees < 1 || trustees > 256) return R::Err(PZ_ERR_INVALID, "deal_shamir: trustees outside 1 .. 256");
    if (threshold < 1 || threshold > trustees) return R::Err(PZ_ERR_INVALID, "deal_shamir: threshold outside 1 .. trustees");
    if (p < BigUint(3) || q < BigUint(3) || p == q || !p.bit(0) || !q.bit(0)) return R::Err(PZ_ERR_INVALID, "deal_shamir: p and q must be distinct odd primes");
    if (!(BigUint(trustees) < p) || !(BigUint(trustees) < q)) return R::Err(PZ_ERR_INVALID, "deal_shamir: the primes must exceed the number of trustees");
    const BigUint n = p * q, n2 = n * n, p1 = p - one, q1 = q - one;
    if (BigUint::gcd(n, p1 * q1) != one) return R::Err(PZ_ERR_INVALID, "deal_shamir: gcd(n, phi(n)) != 1");
    const BigUint lambda = (p1 * q1) / BigUint::gcd(p1, q1), N = n * lambda, theta = lambda * BigUint::mod_inverse(lambda, n);
    DealtShamir out;
    out.key.n = n;
    out.key.g = g_in ? *g_in : n + one;
    out.key.trustees = trustees;
    out.key.threshold = threshold;
    if (out.key.g.is_zero() || !(out.key.g < n2)) return R::Err(PZ_ERR_INVALID, "deal_shamir: g outside (0, n^2)");
    const std::vector<BigUint> unit{one};
    auto power = [&](const BigUint& base, const BigUint& e) { return chip.partial_decrypt(ctx, n, base, e, unit); };   // base^e mod n^2
    auto gt = power(out.key.g, theta);
    if (!gt.ok) return R::Err(gt.err.status, gt.err.msg);
    BigUint a, rem, delta(1);
    BigUint::divmod(gt.val.h, n, a, rem);
    if (rem != one || BigUint::gcd(a % n, n) != one) return R::Err(PZ_ERR_INVALID, "deal_shamir: n does not divide the order of g");
    for (size_t f = 2; f <= trustees; ++f) delta = delta.mul_small(f) % n;
    out.key.mu2 = BigUint::mod_inverse((((two * a) % n) * delta) % n, n);
    std::vector<BigUint> coeffs{theta % N};
    for (size_t k = 1; k < threshold; ++k) coeffs.push_back(rand(N) % N);
    for (size_t i = 1; i <= trustees; ++i) {
        BigUint s;
        for (size_t k = coeffs.size(); k-- > 0;) s = BigUint::reduce_near(s.mul_small(i) + coeffs[k], N, 9);   // s i + a < 257 N < N 2^10
        out.shares.push_back(s);
    }
    const BigUint pp = p1 / two, qq = q1 / two, half = N / two;
    for (;;) {
        const BigUint w = rand(n2) % n2;
        if (w < two || BigUint::gcd(w, n) != one) continue;
        const BigUint v = paillier_add_native(ctx, n, w, w);   // w^2 mod n^2
        if (v == one) continue;
        bool good = true;
        if (safe_primes) {
            auto full = power(v, half);
            if (!full.ok) return R::Err(full.err.status, full.err.msg);
            good = full.val.h == one;
            for (const BigUint* l : {&p, &q, &pp, &qq}) {
                if (!good) break;
                auto part = power(v, half / *l);
                if (!part.ok) return R::Err(part.err.status, part.err.msg);
                good = part.val.h != one;
            }
        }
        if (good) {
            out.key.v = v;
            break;
        }
    }
    out.key.v_order_proved = safe_primes;
    for (const BigUint& s : out.shares) {
        auto h = power(out.key.v, s);
        if (!h.ok) return R::Err(h.err.status, h.err.msg);
        out.key.hs.push_back(h.val.h);
    }
    return R::Ok(out);
}

// Prime generation (keys.py::generate_prime / generate_key are the same in Python integers).  rand(k): uniform in
// [0, k), from the caller's CSPRNG, as in deal_shares.  The search itself runs on the device: there is no host primality test.
inline std::vector<uint64_t> prime_bases(unsigned rounds, const std::function<BigUint(const BigUint&)>& rand) {
    std::vector<uint64_t> out;
    for (unsigned k = 0; k < rounds; ++k) out.push_back(rand(BigUint(1) << 64).to_limbs(1)[0] | 2);
    return out;
}
// offsets one search covers, as keys.default_window: a power of two in 2^10 .. 2^20 around 4 bits (plain) or bits^2 / 8 (safe)
inline size_t prime_default_window(unsigned bits, bool safe) {
    const size_t want = safe ? (size_t)bits * bits / 8 : 4 * (size_t)bits;
    size_t w = 1 << 10;
    while (w < want && w < ((size_t)1 << 20)) w <<= 1;
    return w;
}
// a probable prime of exactly `bits` (40 .. 2048) bits with its two top bits set; with safe, (p - 1) / 2 is a probable prime too.  Per
// window a fresh start (top two bits and the residue forced: odd, or 3 mod 4 with safe) and fresh bases rand(2^64) | 2; the loop draws
// again until a window yields a prime.  window = 0: prime_default_window.
inline Result<BigUint> generate_prime(Context& ctx, const PaillierChip& chip, unsigned bits, bool safe, unsigned rounds,
                                      const std::function<BigUint(const BigUint&)>& rand, size_t window = 0) {
    using R = Result<BigUint>;
    if (bits < 40 || bits > 2048) return R::Err(PZ_ERR_INVALID, "generate_prime: bits outside 40 .. 2048");
    if (rounds < 1 || rounds > 64) return R::Err(PZ_ERR_INVALID, "generate_prime: rounds outside 1 .. 64");
    if (window > ((size_t)1 << 20)) return R::Err(PZ_ERR_INVALID, "generate_prime: window above 2^20");
    const uint64_t stride = safe ? 4 : 2, residue = safe ? 3 : 1;
    if (window == 0) window = prime_default_window(bits, safe);
    const size_t limbs = (bits + 63) / 64;
    const BigUint top = BigUint(3) << (bits - 2), bound = BigUint(1) << bits;
    for (;;) {
        std::vector<uint64_t> w = (rand(BigUint(1) << (bits - 2)) + top).to_limbs(limbs);
        w[0] = (w[0] & ~(stride - 1)) | residue;
        const BigUint start = BigUint::from_limbs(w.data(), limbs);
        if (!(start + BigUint(stride * (window - 1)) < bound)) continue;   // the window would leave the bit length: draw again
        auto offs = chip.prime_search(ctx, start, limbs, window, safe, prime_bases(rounds, rand), 1);
        if (!offs.ok) return R::Err(offs.err.status, offs.err.msg);
        if (!offs.val.empty()) return R::Ok(start + BigUint(stride * offs.val[0]));
    }
}
// (p, q) for deal_shares / deal_shamir: p != q of bits / 2 and bits - bits / 2 bits, n = p q of exactly `bits` bits, gcd(n, phi(n)) = 1;
// with safe both are safe primes (and (p - 1) / 2 != (q - 1) / 2 follows), which is what the dealers' safe_primes argument asserts
struct PrimePair {
    BigUint p, q;
};
inline Result<PrimePair> generate_key(Context& ctx, const PaillierChip& chip, unsigned bits, bool safe, unsigned rounds,
                                      const std::function<BigUint(const BigUint&)>& rand, size_t window = 0) {
    using R = Result<PrimePair>;
    const BigUint one(1);
    for (;;) {
        auto p = generate_prime(ctx, chip, bits / 2, safe, rounds, rand, window);
        if (!p.ok) return R::Err(p.err.status, p.err.msg);
        auto q = generate_prime(ctx, chip, bits - bits / 2, safe, rounds, rand, window);
        if (!q.ok) return R::Err(q.err.status, q.err.msg);
        const BigUint n = p.val * q.val;
        if (p.val != q.val && n.bits() == bits && BigUint::gcd(n, (p.val - one) * (q.val - one)) == one) return R::Ok(PrimePair{p.val, q.val});
    }
}
// what a caller of deal_shares / deal_shamir passes as safe_primes: p, q, (p - 1) / 2 and (q - 1) / 2 all pass `rounds` rounds on the
// device over fresh bases, and p != q
inline Result<bool> primes_are_safe(Context& ctx, const PaillierChip& chip, const BigUint& p, const BigUint& q, unsigned rounds,
                                    const std::function<BigUint(const BigUint&)>& rand) {
    using R = Result<bool>;
    if (rounds < 1 || rounds > 64) return R::Err(PZ_ERR_INVALID, "primes_are_safe: rounds outside 1 .. 64");
    if (p < BigUint(5) || q < BigUint(5) || p == q) return R::Ok(false);
    const BigUint one(1), two(2);
    auto res = chip.is_probable_prime(ctx, {p, q, (p - one) / two, (q - one) / two}, prime_bases(rounds, rand));
    if (!res.ok) return R::Err(res.err.status, res.err.msg);
    return R::Ok(res.val[0] && res.val[1] && res.val[2] && res.val[3]);
}

// paillier.rs:87-92: (g^m * r^n) mod n^2 -- one pz_paillier_encrypt call without a trace
inline BigUint paillier_enc_native(Context& ctx, const BigUint& n, const BigUint& g, const BigUint& m, const BigUint& r) {
    size_t Ln = std::max<size_t>(1, std::max(std::max(n.l.size(), g.l.size()), std::max(m.l.size(), r.l.size())));
    std::vector<uint64_t> nv = n.to_limbs(Ln), gv = g.to_limbs(Ln), mv = m.to_limbs(Ln), rv = r.to_limbs(Ln), c(2 * Ln);
    int rc = pz_paillier_encrypt(ctx.raw(), (uint32_t)Ln, 1, nv.data(), gv.data(), mv.data(), rv.data(), nullptr, 0, nullptr,
                                 nullptr, c.data());
    if (rc != PZ_OK) throw std::runtime_error(std::string("paillier_enc_native: ") + pz_strerror(rc));  // Rust: % 0 panics
    return BigUint::from_limbs(c.data(), 2 * Ln);
}
// paillier.rs:94-97
inline BigUint paillier_add_native(Context& ctx, const BigUint& n, const BigUint& c1, const BigUint& c2) {
    BigUint n2 = n * n;
    size_t L = std::max<size_t>(1, std::max(n2.l.size(), std::max(c1.l.size(), c2.l.size())));
    std::vector<uint64_t> nv = n2.to_limbs(L), a = c1.to_limbs(L), b = c2.to_limbs(L), q(L), r(L);
    int rc = pz_mul_mod(ctx.raw(), (uint32_t)L, a.data(), b.data(), nv.data(), q.data(), r.data());
    if (rc != PZ_OK) throw std::runtime_error(std::string("paillier_add_native: ") + pz_strerror(rc));
    return BigUint::from_limbs(r.data(), L);
}

// bench.rs:11-31
struct PaillierEncryptionInput {
    unsigned enc_bits, limb_bits;
    BigUint n, g, m, r, res;
};
struct PaillierAddCipherInput {
    unsigned limb_bits, enc_bits;
    BigUint n, g, c1, c2, res;
};

// bench.rs:33-75: assign n, g, m, r -> encrypt -> assign res at 2*enc_bits -> value assert -> assert_equal_fresh
inline void paillier_enc_test(Context& ctx, const RangeChip& range, const PaillierEncryptionInput& input) {
    BigUintChip biguint_chip = BigUintChip::construct(&range, input.limb_bits);
    PaillierChip paillier_chip = PaillierChip::construct(&biguint_chip, input.enc_bits);
    auto n_assigned = biguint_chip.assign_integer(ctx, input.n, input.enc_bits).unwrap();
    auto g_assigned = biguint_chip.assign_integer(ctx, input.g, input.enc_bits).unwrap();
    EncryptionPublicKeyAssigned pk_enc{n_assigned, g_assigned};
    auto m_assigned = biguint_chip.assign_integer(ctx, input.m, input.enc_bits).unwrap();
    auto r_assigned = biguint_chip.assign_integer(ctx, input.r, input.enc_bits).unwrap();
    auto c_assigned = paillier_chip.encrypt(ctx, pk_enc, m_assigned, r_assigned).unwrap();
    auto res_assigned = biguint_chip.assign_integer(ctx, input.res, input.enc_bits * 2).unwrap();
    if (c_assigned.value() != res_assigned.value()) throw std::runtime_error("assertion failed: `(left == right)` (paillier_enc_test)");
    biguint_chip.assert_equal_fresh(ctx, c_assigned, res_assigned).unwrap();
}
// bench.rs:77-117
inline void paillier_enc_add_test(Context& ctx, const RangeChip& range, const PaillierAddCipherInput& input) {
    BigUintChip biguint_chip = BigUintChip::construct(&range, input.limb_bits);
    PaillierChip paillier_chip = PaillierChip::construct(&biguint_chip, input.enc_bits);
    auto n_assigned = biguint_chip.assign_integer(ctx, input.n, input.enc_bits).unwrap();
    auto g_assigned = biguint_chip.assign_integer(ctx, input.g, input.enc_bits).unwrap();
    EncryptionPublicKeyAssigned pk_enc{n_assigned, g_assigned};
    auto c1_assigned = biguint_chip.assign_integer(ctx, input.c1, input.enc_bits).unwrap();
    auto c2_assigned = biguint_chip.assign_integer(ctx, input.c2, input.enc_bits).unwrap();
    auto res = paillier_chip.add(ctx, pk_enc, c1_assigned, c2_assigned).unwrap();
    auto res_assigned = biguint_chip.assign_integer(ctx, input.res, input.enc_bits * 2).unwrap();
    if (res.value() != res_assigned.value()) throw std::runtime_error("assertion failed: `(left == right)` (paillier_enc_add_test)");
    biguint_chip.assert_equal_fresh(ctx, res, res_assigned).unwrap();
}

// the tally's driver beside the reference's two: assign n, assign every c_i at 2 * enc_bits, tally, assign res, assert_equal_fresh
struct PaillierTallyInput {
    unsigned limb_bits, enc_bits;
    BigUint n;
    std::vector<BigUint> cts;
    BigUint res;
};
inline void paillier_tally_test(Context& ctx, const RangeChip& range, const PaillierTallyInput& input) {
    BigUintChip biguint_chip = BigUintChip::construct(&range, input.limb_bits);
    PaillierChip paillier_chip = PaillierChip::construct(&biguint_chip, input.enc_bits);
    auto n_assigned = biguint_chip.assign_integer(ctx, input.n, input.enc_bits).unwrap();
    EncryptionPublicKeyAssigned pk_enc{n_assigned, {}};   // g plays no part in an addition
    std::vector<AssignedBigUint<Fresh>> cts;
    for (const BigUint& c : input.cts) cts.push_back(biguint_chip.assign_integer(ctx, c, input.enc_bits * 2).unwrap());
    auto root = paillier_chip.tally(ctx, pk_enc, cts).unwrap();
    auto res_assigned = biguint_chip.assign_integer(ctx, input.res, input.enc_bits * 2).unwrap();
    if (root.value() != res_assigned.value()) throw std::runtime_error("assertion failed: `(left == right)` (paillier_tally_test)");
    biguint_chip.assert_equal_fresh(ctx, root, res_assigned).unwrap();
}

// the weighted tally's driver: assign n, assign every c_i at 2 * enc_bits, load_witness every w_i, weighted_tally, assign res,
// assert_equal_fresh
struct PaillierWTallyInput {
    unsigned limb_bits, enc_bits, w_bits;
    BigUint n;
    std::vector<BigUint> cts;
    std::vector<uint64_t> weights;
    BigUint res;
};
inline void paillier_wtally_test(Context& ctx, const RangeChip& range, const PaillierWTallyInput& input) {
    BigUintChip biguint_chip = BigUintChip::construct(&range, input.limb_bits);
    PaillierChip paillier_chip = PaillierChip::construct(&biguint_chip, input.enc_bits);
    auto n_assigned = biguint_chip.assign_integer(ctx, input.n, input.enc_bits).unwrap();
    EncryptionPublicKeyAssigned pk_enc{n_assigned, {}};   // g plays no part here
    std::vector<AssignedBigUint<Fresh>> cts;
    for (const BigUint& c : input.cts) cts.push_back(biguint_chip.assign_integer(ctx, c, input.enc_bits * 2).unwrap());
    std::vector<AssignedWeight> weights;
    for (uint64_t w : input.weights) weights.push_back(AssignedWeight{w, ctx.load_witness()});
    auto root = paillier_chip.weighted_tally(ctx, pk_enc, cts, weights, input.w_bits).unwrap();
    auto res_assigned = biguint_chip.assign_integer(ctx, input.res, input.enc_bits * 2).unwrap();
    if (root.value() != res_assigned.value()) throw std::runtime_error("assertion failed: `(left == right)` (paillier_wtally_test)");
    biguint_chip.assert_equal_fresh(ctx, root, res_assigned).unwrap();
}

// the ballot's driver: assign n, g, load_witness every m_i, for K >= 2 their sum, assign every r_i, ballot, then per ciphertext assign
// res_i and assert_equal_fresh
struct PaillierBallotInput {
    unsigned limb_bits, enc_bits, m_bits;
    BigUint n, g;
    std::vector<uint64_t> ms;
    std::vector<BigUint> rs, res;
};
inline void paillier_ballot_test(Context& ctx, const RangeChip& range, const PaillierBallotInput& input) {
    BigUintChip biguint_chip = BigUintChip::construct(&range, input.limb_bits);
    PaillierChip paillier_chip = PaillierChip::construct(&biguint_chip, input.enc_bits);
    auto n_assigned = biguint_chip.assign_integer(ctx, input.n, input.enc_bits).unwrap();
    auto g_assigned = biguint_chip.assign_integer(ctx, input.g, input.enc_bits).unwrap();
    EncryptionPublicKeyAssigned pk_enc{n_assigned, g_assigned};
    std::vector<AssignedWeight> ms;
    for (uint64_t m : input.ms) ms.push_back(AssignedWeight{m, ctx.load_witness()});
    if (ms.size() >= 2) ctx.sum(ms.size());
    std::vector<AssignedBigUint<Fresh>> rs;
    for (const BigUint& r : input.rs) rs.push_back(biguint_chip.assign_integer(ctx, r, input.enc_bits).unwrap());
    auto cts = paillier_chip.ballot(ctx, pk_enc, ms, rs, input.m_bits).unwrap();
    if (cts.size() != input.res.size()) throw std::runtime_error("paillier_ballot_test: one expected ciphertext per message");
    for (size_t i = 0; i < cts.size(); ++i) {
        auto res_assigned = biguint_chip.assign_integer(ctx, input.res[i], input.enc_bits * 2).unwrap();
        if (cts[i].value() != res_assigned.value()) throw std::runtime_error("assertion failed: `(left == right)` (paillier_ballot_test)");
        biguint_chip.assert_equal_fresh(ctx, cts[i], res_assigned).unwrap();
    }
}

// the short-randomness ballot's driver: assign n, g, hs at full width, load_witness every m_i, for K >= 2 their sum, assign every s_i on
// s_limbs limbs, sballot, then per ciphertext assign res_i and assert_equal_fresh
struct PaillierSBallotInput {
    unsigned limb_bits, enc_bits, m_bits, s_limbs;
    BigUint n, g, hs;
    std::vector<uint64_t> ms;
    std::vector<BigUint> ss, res;
};
inline void paillier_sballot_test(Context& ctx, const RangeChip& range, const PaillierSBallotInput& input) {
    BigUintChip biguint_chip = BigUintChip::construct(&range, input.limb_bits);
    PaillierChip paillier_chip = PaillierChip::construct(&biguint_chip, input.enc_bits);
    auto n_assigned = biguint_chip.assign_integer(ctx, input.n, input.enc_bits).unwrap();
    auto g_assigned = biguint_chip.assign_integer(ctx, input.g, input.enc_bits).unwrap();
    auto hs_assigned = biguint_chip.assign_integer(ctx, input.hs, input.enc_bits * 2).unwrap();
    EncryptionPublicKeyAssigned pk_enc{n_assigned, g_assigned};
    std::vector<AssignedWeight> ms;
    for (uint64_t m : input.ms) ms.push_back(AssignedWeight{m, ctx.load_witness()});
    if (ms.size() >= 2) ctx.sum(ms.size());
    std::vector<AssignedBigUint<Fresh>> ss;
    for (const BigUint& s : input.ss) ss.push_back(biguint_chip.assign_integer(ctx, s, input.s_limbs * input.limb_bits).unwrap());
    auto cts = paillier_chip.sballot(ctx, pk_enc, hs_assigned, ms, ss, input.m_bits).unwrap();
    if (cts.size() != input.res.size()) throw std::runtime_error("paillier_sballot_test: one expected ciphertext per message");
    for (size_t i = 0; i < cts.size(); ++i) {
        auto res_assigned = biguint_chip.assign_integer(ctx, input.res[i], input.enc_bits * 2).unwrap();
        if (cts[i].value() != res_assigned.value()) throw std::runtime_error("assertion failed: `(left == right)` (paillier_sballot_test)");
        biguint_chip.assert_equal_fresh(ctx, cts[i], res_assigned).unwrap();
    }
}

// the element hs that short-randomness ("DJN mode") encryption adds to a public key (keys.py::djn_generator is
// the same in Python): hs = (-x^2 mod n)^n mod n^2 for a unit x drawn with rand (rand(k): uniform in [0, k), from the caller's CSPRNG),
// the power taken on the device by PaillierChip::partial_decrypt's chain.  Security of c = g^m hs^s with a short s rests on the
// short-exponent assumption in <hs>; the scheme asks for p = q = 3 (mod 4) (pz::generate_key with safe gives such primes).  Refuses an
// even or tiny n (PZ_ERR_INVALID).
inline Result<BigUint> djn_generator(Context& ctx, const PaillierChip& chip, const BigUint& n, const std::function<BigUint(const BigUint&)>& rand) {
    using R = Result<BigUint>;
    const BigUint one(1), two(2);
    if (n < BigUint(15) || !n.bit(0)) return R::Err(PZ_ERR_INVALID, "djn_generator: n must be an odd modulus");
    BigUint x;
    do x = rand(n) % n;
    while (x < two || BigUint::gcd(x, n) != one);
    const BigUint h = (n - (x * x) % n) % n;
    auto p = chip.partial_decrypt(ctx, n, h, n, std::vector<BigUint>{one});   // h^n mod n^2
    if (!p.ok) return R::Err(p.err.status, p.err.msg);
    return R::Ok(p.val.h);
}

// the packed ballot's driver: assign n, hs and the K slot bases at full width, load_witness every v_ij (ciphertext-major), for K >= 2 one
// sum per ciphertext, assign every s_i on s_limbs limbs, pballot, then per ciphertext assign res_i and assert_equal_fresh
struct PaillierPBallotInput {
    unsigned limb_bits, enc_bits, m_bits, s_limbs;
    BigUint n, hs;
    std::vector<BigUint> gs;                   // G_0 .. G_{K-1}
    std::vector<std::vector<uint64_t>> vs;     // [R][K]
    std::vector<BigUint> ss, res;
};
inline void paillier_pballot_test(Context& ctx, const RangeChip& range, const PaillierPBallotInput& input) {
    BigUintChip biguint_chip = BigUintChip::construct(&range, input.limb_bits);
    PaillierChip paillier_chip = PaillierChip::construct(&biguint_chip, input.enc_bits);
    auto n_assigned = biguint_chip.assign_integer(ctx, input.n, input.enc_bits).unwrap();
    auto hs_assigned = biguint_chip.assign_integer(ctx, input.hs, input.enc_bits * 2).unwrap();
    std::vector<AssignedBigUint<Fresh>> gs;
    for (const BigUint& gj : input.gs) gs.push_back(biguint_chip.assign_integer(ctx, gj, input.enc_bits * 2).unwrap());
    std::vector<std::vector<AssignedWeight>> vs;
    for (const auto& row : input.vs) {
        vs.emplace_back();
        for (uint64_t v : row) vs.back().push_back(AssignedWeight{v, ctx.load_witness()});
    }
    if (gs.size() >= 2)
        for (size_t i = 0; i < vs.size(); ++i) ctx.sum(gs.size());
    std::vector<AssignedBigUint<Fresh>> ss;
    for (const BigUint& s : input.ss) ss.push_back(biguint_chip.assign_integer(ctx, s, input.s_limbs * input.limb_bits).unwrap());
    auto cts = paillier_chip.pballot(ctx, n_assigned, hs_assigned, gs, vs, ss, input.m_bits).unwrap();
    if (cts.size() != input.res.size()) throw std::runtime_error("paillier_pballot_test: one expected ciphertext per row of values");
    for (size_t i = 0; i < cts.size(); ++i) {
        auto res_assigned = biguint_chip.assign_integer(ctx, input.res[i], input.enc_bits * 2).unwrap();
        if (cts[i].value() != res_assigned.value()) throw std::runtime_error("assertion failed: `(left == right)` (paillier_pballot_test)");
        biguint_chip.assert_equal_fresh(ctx, cts[i], res_assigned).unwrap();
    }
}

// the public slot bases of a packed ballot (keys.py::pballot_bases is the same in Python): G_j = g^(2^(j w)) mod
// n^2 for j = 0 .. slots - 1, read from the squaring records of ONE pz_paillier_trace of g^(2^((slots - 1) w)) -- every bit of that
// exponent below its top one is clear, so record t is the square whose remainder is g^(2^(t + 1)) and the remainder of record j w - 1
// is G_j.  Refuses 2^(slots w) > n: the packed plaintext must stay below n (PZ_ERR_INVALID).
inline Result<std::vector<BigUint>> pballot_bases(Context& ctx, const BigUint& n, const BigUint& g, unsigned slots, unsigned slot_bits) {
    using R = Result<std::vector<BigUint>>;
    if (slots < 1 || slot_bits < 1 || n < BigUint(15) || !n.bit(0)) return R::Err(PZ_ERR_INVALID, "pballot_bases: slots, slot_bits >= 1 and an odd modulus");
    if (n < (BigUint(1) << ((size_t)slots * slot_bits))) return R::Err(PZ_ERR_INVALID, "pballot_bases: 2^(slots * slot_bits) exceeds n");
    const BigUint n2 = n * n;
    if (g < BigUint(1) || !(g < n2)) return R::Err(PZ_ERR_INVALID, "pballot_bases: g is in [1, n^2)");
    std::vector<BigUint> out{g};
    const size_t top = (size_t)(slots - 1) * slot_bits;
    if (top == 0) return R::Ok(out);
    const unsigned wn = (unsigned)((n.bits() + 63) / 64), wk = 2 * wn, el = (unsigned)(top / 64 + 1);
    std::vector<uint64_t> nv = n2.to_limbs(wk), gv = g.to_limbs(wk), ev = (BigUint(1) << top).to_limbs(el), res(wk);
    std::vector<uint64_t> steps((top + 2) * 4 * wk);
    size_t ns = top + 2;
    int rc = pz_paillier_trace(ctx.raw(), wk, nv.data(), gv.data(), ev.data(), el, steps.data(), &ns, res.data());
    if (rc != PZ_OK) return R::Err(rc, std::string("pz_paillier_trace: ") + pz_strerror(rc));
    if (ns != top + 2) return R::Err(PZ_ERR_INTERNAL, "pballot_bases: the trace of a power of two has one record per bit and one product");
    for (unsigned j = 1; j < slots; ++j) out.push_back(BigUint::from_limbs(steps.data() + (((size_t)j * slot_bits - 1) * 4 + 3) * wk, wk));
    return R::Ok(out);
}

// the `slots` counts of a decrypted packed total: count j is bits j w .. (j + 1) w of M (keys.py::unpack_tally).  Refuses an M of more
// than slots * slot_bits bits.
inline Result<std::vector<BigUint>> unpack_tally(const BigUint& M, unsigned slots, unsigned slot_bits) {
    using R = Result<std::vector<BigUint>>;
    if (slots < 1 || slot_bits < 1 || M.bits() > (size_t)slots * slot_bits) return R::Err(PZ_ERR_INVALID, "unpack_tally: M has more than slots * slot_bits bits");
    std::vector<BigUint> out;
    for (unsigned j = 0; j < slots; ++j) out.push_back((M >> ((size_t)j * slot_bits)).low_bits(slot_bits));
    return R::Ok(out);
}

// the mix's driver: assign n, every c_j at full width, every r_i, mix, then per output assign res_i and assert_equal_fresh
struct PaillierMixInput {
    unsigned limb_bits, enc_bits;
    BigUint n;
    std::vector<BigUint> cts;
    std::vector<uint32_t> perm;
    std::vector<BigUint> rs, res;
};
inline void paillier_mix_test(Context& ctx, const RangeChip& range, const PaillierMixInput& input, PaillierChip::MixWitness* wit) {
    BigUintChip biguint_chip = BigUintChip::construct(&range, input.limb_bits);
    PaillierChip paillier_chip = PaillierChip::construct(&biguint_chip, input.enc_bits);
    auto n_assigned = biguint_chip.assign_integer(ctx, input.n, input.enc_bits).unwrap();
    std::vector<AssignedBigUint<Fresh>> cts, rs;
    for (const BigUint& c : input.cts) cts.push_back(biguint_chip.assign_integer(ctx, c, input.enc_bits * 2).unwrap());
    for (const BigUint& r : input.rs) rs.push_back(biguint_chip.assign_integer(ctx, r, input.enc_bits).unwrap());
    auto mixed = paillier_chip.mix(ctx, n_assigned, cts, input.perm, rs, wit).unwrap();
    if (mixed.size() != input.res.size()) throw std::runtime_error("paillier_mix_test: one expected output per input");
    for (size_t i = 0; i < mixed.size(); ++i) {
        auto res_assigned = biguint_chip.assign_integer(ctx, input.res[i], input.enc_bits * 2).unwrap();
        if (mixed[i].value() != res_assigned.value()) throw std::runtime_error("assertion failed: `(left == right)` (paillier_mix_test)");
        biguint_chip.assert_equal_fresh(ctx, mixed[i], res_assigned).unwrap();
    }
}

// the short-randomness mix's driver: assign n, hs and every c_j at full width, every s_i on s_limbs limbs, smix, then per output assign
// res_i and assert_equal_fresh
struct PaillierSMixInput {
    unsigned limb_bits, enc_bits, s_limbs;
    BigUint n, hs;
    std::vector<BigUint> cts;
    std::vector<uint32_t> perm;
    std::vector<BigUint> ss, res;
};
inline void paillier_smix_test(Context& ctx, const RangeChip& range, const PaillierSMixInput& input, PaillierChip::MixWitness* wit) {
    BigUintChip biguint_chip = BigUintChip::construct(&range, input.limb_bits);
    PaillierChip paillier_chip = PaillierChip::construct(&biguint_chip, input.enc_bits);
    auto n_assigned = biguint_chip.assign_integer(ctx, input.n, input.enc_bits).unwrap();
    auto hs_assigned = biguint_chip.assign_integer(ctx, input.hs, input.enc_bits * 2).unwrap();
    std::vector<AssignedBigUint<Fresh>> cts, ss;
    for (const BigUint& c : input.cts) cts.push_back(biguint_chip.assign_integer(ctx, c, input.enc_bits * 2).unwrap());
    for (const BigUint& s : input.ss) ss.push_back(biguint_chip.assign_integer(ctx, s, input.s_limbs * input.limb_bits).unwrap());
    auto mixed = paillier_chip.smix(ctx, n_assigned, hs_assigned, cts, input.perm, ss, wit).unwrap();
    if (mixed.size() != input.res.size()) throw std::runtime_error("paillier_smix_test: one expected output per input");
    for (size_t i = 0; i < mixed.size(); ++i) {
        auto res_assigned = biguint_chip.assign_integer(ctx, input.res[i], input.enc_bits * 2).unwrap();
        if (mixed[i].value() != res_assigned.value()) throw std::runtime_error("assertion failed: `(left == right)` (paillier_smix_test)");
        biguint_chip.assert_equal_fresh(ctx, mixed[i], res_assigned).unwrap();
    }
}

// decryption's driver: make the key handle, decrypt every ciphertext, hold the plaintexts to the expected ones and every recovered
// (m, r) to its ciphertext by re-encrypting it (paillier_enc_native) -- throws on any mismatch, like the drivers above
struct PaillierDecryptionInput {
    BigUint n, g, lambda, d;
    std::vector<BigUint> cts, ms;
};
inline void paillier_decrypt_test(Context& ctx, const RangeChip& range, const PaillierDecryptionInput& input) {
    BigUintChip biguint_chip = BigUintChip::construct(&range, 64);
    PaillierChip paillier_chip = PaillierChip::construct(&biguint_chip, (unsigned)input.n.bits());
    auto sk = PaillierSecretKey::create(ctx, input.n, input.g, input.lambda, input.d).unwrap();
    std::vector<Decryption> dec = paillier_chip.decrypt(ctx, *sk, input.cts).unwrap();
    std::vector<Decryption> plain = paillier_chip.decrypt(ctx, *sk, input.cts, false).unwrap();
    if (dec.size() != input.ms.size()) throw std::runtime_error("paillier_decrypt_test: one expected plaintext per ciphertext");
    for (size_t i = 0; i < dec.size(); ++i) {
        if (!dec[i].unit || dec[i].m != input.ms[i] || plain[i].m != input.ms[i])
            throw std::runtime_error("assertion failed: `(left == right)` (paillier_decrypt_test: plaintext)");
        if (paillier_enc_native(ctx, input.n, input.g, dec[i].m, dec[i].r) != input.cts[i])
            throw std::runtime_error("assertion failed: `(left == right)` (paillier_decrypt_test: re-encryption)");
    }
}

// CRT decryption's driver: the handle from the primes keeps its lambda path; the CRT path, the lambda path and the expected plaintexts
// agree entry for entry (m, r and the unit flag), with and without r, and every (m, r) re-encrypts to its ciphertext.  With the primes
// swapped the results are the same.  Throws on any mismatch.
struct PaillierDecryptionCrtInput {
    BigUint n, g, lambda, d, p, q;
    std::vector<BigUint> cts, ms;
};
inline void paillier_decrypt_crt_test(Context& ctx, const RangeChip& range, const PaillierDecryptionCrtInput& input) {
    BigUintChip biguint_chip = BigUintChip::construct(&range, 64);
    PaillierChip paillier_chip = PaillierChip::construct(&biguint_chip, (unsigned)input.n.bits());
    auto sk = PaillierSecretKey::create_crt(ctx, input.n, input.g, input.lambda, input.d, input.p, input.q).unwrap();
    auto swapped = PaillierSecretKey::create_crt(ctx, input.n, input.g, input.lambda, input.d, input.q, input.p).unwrap();
    if (!sk->has_crt() || !swapped->has_crt()) throw std::runtime_error("paillier_decrypt_crt_test: the handle has no CRT part");
    std::vector<Decryption> crt = paillier_chip.decrypt(ctx, *sk, input.cts, true, CrtPath::Yes).unwrap();
    std::vector<Decryption> lam = paillier_chip.decrypt(ctx, *sk, input.cts, true, CrtPath::No).unwrap();
    std::vector<Decryption> plain = paillier_chip.decrypt(ctx, *sk, input.cts, false, CrtPath::Yes).unwrap();
    std::vector<Decryption> other = paillier_chip.decrypt(ctx, *swapped, input.cts).unwrap();
    if (crt.size() != input.ms.size()) throw std::runtime_error("paillier_decrypt_crt_test: one expected plaintext per ciphertext");
    for (size_t i = 0; i < crt.size(); ++i) {
        if (!crt[i].unit || crt[i].m != input.ms[i] || plain[i].m != input.ms[i])
            throw std::runtime_error("assertion failed: `(left == right)` (paillier_decrypt_crt_test: plaintext)");
        if (crt[i].m != lam[i].m || crt[i].r != lam[i].r || crt[i].unit != lam[i].unit)
            throw std::runtime_error("assertion failed: `(left == right)` (paillier_decrypt_crt_test: the CRT path against the lambda path)");
        if (crt[i].m != other[i].m || crt[i].r != other[i].r || crt[i].unit != other[i].unit)
            throw std::runtime_error("assertion failed: `(left == right)` (paillier_decrypt_crt_test: swapped primes)");
        if (paillier_enc_native(ctx, input.n, input.g, crt[i].m, crt[i].r) != input.cts[i])
            throw std::runtime_error("assertion failed: `(left == right)` (paillier_decrypt_crt_test: re-encryption)");
    }
}

// K4 over the mul_mod steps alone (the bulk of the stream; the caller places the buffers)
inline int synthesize_witness(Context& ctx, const RangeChip& range, uint64_t* d_steps, uint64_t* d_modulus, uint64_t* d_advice,
                              uint64_t* d_lookup) {
    return pz_witness_expand_dev(ctx.raw(), ctx.limbs(), ctx.limb_bits(), range.lookup_bits, d_steps, ctx.n_steps(), d_modulus, d_advice,
                                 d_lookup);
}

// The whole tape of one of the two drivers expanded on the device (pz_circuit_expand_dev).  kind 0 = paillier_enc_test
// (x, y = m, r), 1 = paillier_enc_add_test (x, y = c1, c2).  The tape must have the driver's shape; its cell total equals
// pz_circuit_cells (checked).  d_steps / d_modulus / d_advice / d_lookup: device buffers of the caller.
inline int synthesize_circuit(Context& ctx, int kind, unsigned enc_bits, const BigUint& n, const BigUint& g, const BigUint& x,
                              const BigUint& y, const BigUint& res, size_t n_steps_g, size_t n_steps_r, uint64_t* d_steps,
                              uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup) {
    const unsigned W = ctx.limb_bits(), Ln = enc_bits / W, wn = (Ln * W + 63) / 64, wr = (2 * Ln * W + 63) / 64;
    size_t a = 0, l = 0;
    int rc = pz_circuit_cells(kind, Ln, W, ctx.lookup_bits(), n_steps_g, n_steps_r, &a, &l);
    if (rc != PZ_OK) return rc;
    if (a != ctx.advice_cells() || l != ctx.lookup_cells()) return PZ_ERR_INVALID;   // the tape is not this driver's
    std::vector<uint64_t> in;
    for (const BigUint* v : {&n, &g, &x, &y}) {
        std::vector<uint64_t> w = v->to_limbs(wn);
        in.insert(in.end(), w.begin(), w.end());
    }
    std::vector<uint64_t> w = res.to_limbs(wr);
    in.insert(in.end(), w.begin(), w.end());
    return pz_circuit_expand_dev(ctx.raw(), kind, Ln, W, ctx.lookup_bits(), in.data(), d_steps, n_steps_g, n_steps_r, d_modulus,
                                 d_advice, d_lookup, 0, 0);
}

// the tally's tape (paillier_tally_test) expanded on the device: circuit kind 3, inputs n | c_1 .. c_B | res
inline int synthesize_tally_circuit(Context& ctx, unsigned enc_bits, const BigUint& n, const std::vector<BigUint>& cts, const BigUint& res,
                                    uint64_t* d_steps, uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup) {
    const unsigned W = ctx.limb_bits(), Ln = enc_bits / W, wn = (Ln * W + 63) / 64, wr = (2 * Ln * W + 63) / 64;
    if (cts.size() < 2 || ctx.n_steps() != cts.size() - 1) return PZ_ERR_INVALID;
    size_t a = 0, l = 0;
    int rc = pz_circuit_cells(3, Ln, W, ctx.lookup_bits(), cts.size() - 1, 0, &a, &l);
    if (rc != PZ_OK) return rc;
    if (a != ctx.advice_cells() || l != ctx.lookup_cells()) return PZ_ERR_INVALID;   // the tape is not this driver's
    std::vector<uint64_t> in = n.to_limbs(wn);
    for (const BigUint& c : cts) {
        std::vector<uint64_t> w = c.to_limbs(wr);
        in.insert(in.end(), w.begin(), w.end());
    }
    std::vector<uint64_t> w = res.to_limbs(wr);
    in.insert(in.end(), w.begin(), w.end());
    return pz_circuit_expand_dev(ctx.raw(), 3, Ln, W, ctx.lookup_bits(), in.data(), d_steps, cts.size() - 1, 0, d_modulus, d_advice,
                                 d_lookup, 0, 0);
}

// the weighted tally's tape (paillier_wtally_test) expanded on the device: circuit kind 4, inputs n | c_1 .. c_B | w_1 .. w_B | res
inline int synthesize_wtally_circuit(Context& ctx, unsigned enc_bits, unsigned w_bits, const BigUint& n, const std::vector<BigUint>& cts,
                                     const std::vector<uint64_t>& weights, const BigUint& res, uint64_t* d_steps, uint64_t* d_modulus,
                                     uint64_t* d_advice, uint64_t* d_lookup) {
    const unsigned W = ctx.limb_bits(), Ln = enc_bits / W, wn = (Ln * W + 63) / 64, wr = (2 * Ln * W + 63) / 64;
    const size_t B = cts.size(), ng = 2 * B * w_bits;
    if (B < 1 || weights.size() != B || ctx.n_steps() != ng + B - 1) return PZ_ERR_INVALID;
    size_t a = 0, l = 0;
    int rc = pz_circuit_cells(4, Ln, W, ctx.lookup_bits(), ng, B - 1, &a, &l);
    if (rc != PZ_OK) return rc;
    if (a != ctx.advice_cells() || l != ctx.lookup_cells()) return PZ_ERR_INVALID;   // the tape is not this driver's
    std::vector<uint64_t> in = n.to_limbs(wn);
    for (const BigUint& c : cts) {
        std::vector<uint64_t> w = c.to_limbs(wr);
        in.insert(in.end(), w.begin(), w.end());
    }
    in.insert(in.end(), weights.begin(), weights.end());
    std::vector<uint64_t> w = res.to_limbs(wr);
    in.insert(in.end(), w.begin(), w.end());
    return pz_circuit_expand_dev(ctx.raw(), 4, Ln, W, ctx.lookup_bits(), in.data(), d_steps, ng, B - 1, d_modulus, d_advice, d_lookup, 0, 0);
}

// the ballot's tape (paillier_ballot_test) expanded on the device: circuit kind 6, inputs n | g | m_1 .. m_K | r_1 .. r_K | res_1 .. res_K
inline int synthesize_ballot_circuit(Context& ctx, unsigned enc_bits, unsigned m_bits, size_t n_steps_r, const BigUint& n, const BigUint& g,
                                     const std::vector<uint64_t>& ms, const std::vector<BigUint>& rs, const std::vector<BigUint>& res,
                                     uint64_t* d_steps, uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup) {
    const unsigned W = ctx.limb_bits(), Ln = enc_bits / W, wn = (Ln * W + 63) / 64, wr = (2 * Ln * W + 63) / 64;
    const size_t K = ms.size();
    if (K < 1 || rs.size() != K || res.size() != K || ctx.n_steps() != K * (2 * (size_t)m_bits + n_steps_r + 1)) return PZ_ERR_INVALID;
    size_t a = 0, l = 0;
    int rc = pz_ballot_cells(Ln, W, ctx.lookup_bits(), K, m_bits, n_steps_r, &a, &l);
    if (rc != PZ_OK) return rc;
    if (a != ctx.advice_cells() || l != ctx.lookup_cells()) return PZ_ERR_INVALID;   // the tape is not this driver's
    std::vector<uint64_t> in = n.to_limbs(wn), w = g.to_limbs(wn);
    in.insert(in.end(), w.begin(), w.end());
    in.insert(in.end(), ms.begin(), ms.end());
    for (const BigUint& r : rs) {
        w = r.to_limbs(wn);
        in.insert(in.end(), w.begin(), w.end());
    }
    for (const BigUint& c : res) {
        w = c.to_limbs(wr);
        in.insert(in.end(), w.begin(), w.end());
    }
    return pz_ballot_expand_dev(ctx.raw(), Ln, W, ctx.lookup_bits(), K, m_bits, n_steps_r, in.data(), d_steps, d_modulus, d_advice, d_lookup, 0, 0);
}

// the mix's tape (paillier_mix_test) expanded on the device: circuit kind 8, inputs n | c_1 .. c_K | r_1 .. r_K | res_1 .. res_K, the switch
// bits and route layers of `wit`.  The records and routes go up with fields of 2 * ceil(Ln W / 64) words, as pz_paillier_mix_dev leaves
// them.  d_work: device memory for both, (K (n_steps_r + 1) 4 + layers K) 2 wn words.
inline int synthesize_mix_circuit(Context& ctx, unsigned enc_bits, size_t n_steps_r, const BigUint& n, const std::vector<BigUint>& cts,
                                  const std::vector<BigUint>& rs, const std::vector<BigUint>& res, const PaillierChip::MixWitness& wit,
                                  uint64_t* d_work, uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup) {
    const unsigned W = ctx.limb_bits(), Ln = enc_bits / W, wn = (Ln * W + 63) / 64, wr = (2 * Ln * W + 63) / 64, wk = 2 * wn;
    const size_t K = cts.size(), per = n_steps_r + 1, layers = benes_layers(K);
    if (!benes_is_count(K) || rs.size() != K || res.size() != K || ctx.n_steps() != K * per || ctx.words() != wr) return PZ_ERR_INVALID;
    if (wit.bits.size() != layers * (K / 2) || wit.routes.size() != layers * K * wk) return PZ_ERR_INVALID;
    size_t a = 0, l = 0;
    int rc = pz_mix_cells(Ln, W, ctx.lookup_bits(), K, n_steps_r, &a, &l);
    if (rc != PZ_OK) return rc;
    if (a != ctx.advice_cells() || l != ctx.lookup_cells()) return PZ_ERR_INVALID;   // the tape is not this driver's
    std::vector<uint64_t> in = n.to_limbs(wn), w;
    for (const BigUint& c : cts) {
        w = c.to_limbs(wr);
        in.insert(in.end(), w.begin(), w.end());
    }
    for (const BigUint& r : rs) {
        w = r.to_limbs(wn);
        in.insert(in.end(), w.begin(), w.end());
    }
    for (const BigUint& c : res) {
        w = c.to_limbs(wr);
        in.insert(in.end(), w.begin(), w.end());
    }
    const std::vector<uint64_t>& tp = ctx.tape();
    std::vector<uint64_t> rec(K * per * 4 * wk, 0);
    for (size_t f = 0; f < K * per * 4; ++f) std::copy(tp.begin() + f * wr, tp.begin() + (f + 1) * wr, rec.begin() + f * wk);
    uint64_t* d_routes = d_work + rec.size();
    rc = pz_upload(ctx.raw(), d_work, rec.data(), rec.size() * 8);
    std::fill(rec.begin(), rec.end(), 0);
    if (rc == PZ_OK && !wit.routes.empty()) rc = pz_upload(ctx.raw(), d_routes, wit.routes.data(), wit.routes.size() * 8);
    if (rc != PZ_OK) return rc;
    return pz_mix_expand_dev(ctx.raw(), Ln, W, ctx.lookup_bits(), K, n_steps_r, in.data(), wit.bits.empty() ? nullptr : wit.bits.data(),
                             layers ? d_routes : nullptr, d_work, d_modulus, d_advice, d_lookup, 0, 0);
}

// the short-randomness ballot's tape (paillier_sballot_test) expanded on the device: circuit kind 9, inputs n | g | hs | m_1 .. m_K |
// s_1 .. s_K | res_1 .. res_K.  The records go up with fields of 2 * ceil(Ln W / 64) words, as pz_paillier_sballot_dev leaves them.
// d_work: device memory for them, K (2 m_bits + 2 s_limbs W + 1) 4 * 2 wn words.
inline int synthesize_sballot_circuit(Context& ctx, unsigned enc_bits, unsigned m_bits, unsigned s_limbs, const BigUint& n, const BigUint& g,
                                      const BigUint& hs, const std::vector<uint64_t>& ms, const std::vector<BigUint>& ss,
                                      const std::vector<BigUint>& res, uint64_t* d_work, uint64_t* d_modulus, uint64_t* d_advice,
                                      uint64_t* d_lookup) {
    const unsigned W = ctx.limb_bits(), Ln = enc_bits / W, wn = (Ln * W + 63) / 64, wr = (2 * Ln * W + 63) / 64, wk = 2 * wn;
    const unsigned sw = (s_limbs * W + 63) / 64;
    const size_t K = ms.size(), per = 2 * (size_t)m_bits + 2 * (size_t)s_limbs * W + 1;
    if (K < 1 || ss.size() != K || res.size() != K || ctx.n_steps() != K * per || ctx.words() != wr) return PZ_ERR_INVALID;
    size_t a = 0, l = 0;
    int rc = pz_sballot_cells(Ln, W, ctx.lookup_bits(), K, m_bits, s_limbs, &a, &l);
    if (rc != PZ_OK) return rc;
    if (a != ctx.advice_cells() || l != ctx.lookup_cells()) return PZ_ERR_INVALID;   // the tape is not this driver's
    std::vector<uint64_t> in = n.to_limbs(wn), w = g.to_limbs(wn);
    in.insert(in.end(), w.begin(), w.end());
    w = hs.to_limbs(wr);
    in.insert(in.end(), w.begin(), w.end());
    in.insert(in.end(), ms.begin(), ms.end());
    for (const BigUint& s : ss) {
        w = s.to_limbs(sw);
        in.insert(in.end(), w.begin(), w.end());
    }
    for (const BigUint& c : res) {
        w = c.to_limbs(wr);
        in.insert(in.end(), w.begin(), w.end());
    }
    const std::vector<uint64_t>& tp = ctx.tape();
    std::vector<uint64_t> rec(K * per * 4 * wk, 0);
    for (size_t f = 0; f < K * per * 4; ++f) std::copy(tp.begin() + f * wr, tp.begin() + (f + 1) * wr, rec.begin() + f * wk);
    rc = pz_upload(ctx.raw(), d_work, rec.data(), rec.size() * 8);
    std::fill(rec.begin(), rec.end(), 0);
    if (rc == PZ_OK)
        rc = pz_sballot_expand_dev(ctx.raw(), Ln, W, ctx.lookup_bits(), K, m_bits, s_limbs, in.data(), d_work, d_modulus, d_advice, d_lookup, 0, 0);
    std::fill(in.begin(), in.end(), 0);
    return rc;
}

// the packed ballot's tape (paillier_pballot_test) expanded on the device: circuit kind 11, inputs n | hs | G_0 .. G_{K-1} | v_11 .. v_RK |
// s_1 .. s_R | res_1 .. res_R.  The records go up with fields of 2 * ceil(Ln W / 64) words, as pz_paillier_pballot_dev leaves them.
// d_work: device memory for them, R (2 m_bits K + 2 s_limbs W + K) 4 * 2 wn words.
inline int synthesize_pballot_circuit(Context& ctx, unsigned enc_bits, unsigned m_bits, unsigned s_limbs, const BigUint& n, const BigUint& hs,
                                      const std::vector<BigUint>& gs, const std::vector<std::vector<uint64_t>>& vs,
                                      const std::vector<BigUint>& ss, const std::vector<BigUint>& res, uint64_t* d_work, uint64_t* d_modulus,
                                      uint64_t* d_advice, uint64_t* d_lookup) {
    const unsigned W = ctx.limb_bits(), Ln = enc_bits / W, wn = (Ln * W + 63) / 64, wr = (2 * Ln * W + 63) / 64, wk = 2 * wn;
    const unsigned sw = (s_limbs * W + 63) / 64;
    const size_t Rn = vs.size(), K = gs.size(), per = 2 * (size_t)m_bits * K + 2 * (size_t)s_limbs * W + K;
    if (Rn < 1 || K < 1 || ss.size() != Rn || res.size() != Rn || ctx.n_steps() != Rn * per || ctx.words() != wr) return PZ_ERR_INVALID;
    size_t a = 0, l = 0;
    int rc = pz_pballot_cells(Ln, W, ctx.lookup_bits(), Rn, (uint32_t)K, m_bits, s_limbs, &a, &l);
    if (rc != PZ_OK) return rc;
    if (a != ctx.advice_cells() || l != ctx.lookup_cells()) return PZ_ERR_INVALID;   // the tape is not this driver's
    std::vector<uint64_t> in = n.to_limbs(wn), w = hs.to_limbs(wr);
    in.insert(in.end(), w.begin(), w.end());
    for (const BigUint& gj : gs) {
        w = gj.to_limbs(wr);
        in.insert(in.end(), w.begin(), w.end());
    }
    for (const auto& row : vs) {
        if (row.size() != K) return PZ_ERR_INVALID;
        in.insert(in.end(), row.begin(), row.end());
    }
    for (const BigUint& s : ss) {
        w = s.to_limbs(sw);
        in.insert(in.end(), w.begin(), w.end());
    }
    for (const BigUint& c : res) {
        w = c.to_limbs(wr);
        in.insert(in.end(), w.begin(), w.end());
    }
    const std::vector<uint64_t>& tp = ctx.tape();
    std::vector<uint64_t> rec(Rn * per * 4 * wk, 0);
    for (size_t f = 0; f < Rn * per * 4; ++f) std::copy(tp.begin() + f * wr, tp.begin() + (f + 1) * wr, rec.begin() + f * wk);
    rc = pz_upload(ctx.raw(), d_work, rec.data(), rec.size() * 8);
    std::fill(rec.begin(), rec.end(), 0);
    if (rc == PZ_OK)
        rc = pz_pballot_expand_dev(ctx.raw(), Ln, W, ctx.lookup_bits(), Rn, (uint32_t)K, m_bits, s_limbs, in.data(), d_work, d_modulus, d_advice,
                                   d_lookup, 0, 0);
    std::fill(in.begin(), in.end(), 0);
    return rc;
}

// the short-randomness mix's tape (paillier_smix_test) expanded on the device: circuit kind 10, inputs n | hs | c_1 .. c_K | s_1 .. s_K |
// res_1 .. res_K, the switch bits and route layers of `wit`.  The records and routes go up with fields of 2 * ceil(Ln W / 64) words, as
// pz_paillier_smix_dev leaves them.  d_work: device memory for both, (K (2 s_limbs W + 1) 4 + layers K) 2 wn words.
inline int synthesize_smix_circuit(Context& ctx, unsigned enc_bits, unsigned s_limbs, const BigUint& n, const BigUint& hs,
                                   const std::vector<BigUint>& cts, const std::vector<BigUint>& ss, const std::vector<BigUint>& res,
                                   const PaillierChip::MixWitness& wit, uint64_t* d_work, uint64_t* d_modulus, uint64_t* d_advice,
                                   uint64_t* d_lookup) {
    const unsigned W = ctx.limb_bits(), Ln = enc_bits / W, wn = (Ln * W + 63) / 64, wr = (2 * Ln * W + 63) / 64, wk = 2 * wn;
    const unsigned sw = (s_limbs * W + 63) / 64;
    const size_t K = cts.size(), per = 2 * (size_t)s_limbs * W + 1, layers = benes_layers(K);
    if (!benes_is_count(K) || ss.size() != K || res.size() != K || ctx.n_steps() != K * per || ctx.words() != wr) return PZ_ERR_INVALID;
    if (wit.bits.size() != layers * (K / 2) || wit.routes.size() != layers * K * wk) return PZ_ERR_INVALID;
    size_t a = 0, l = 0;
    int rc = pz_smix_cells(Ln, W, ctx.lookup_bits(), K, s_limbs, &a, &l);
    if (rc != PZ_OK) return rc;
    if (a != ctx.advice_cells() || l != ctx.lookup_cells()) return PZ_ERR_INVALID;   // the tape is not this driver's
    std::vector<uint64_t> in = n.to_limbs(wn), w = hs.to_limbs(wr);
    in.insert(in.end(), w.begin(), w.end());
    for (const BigUint& c : cts) {
        w = c.to_limbs(wr);
        in.insert(in.end(), w.begin(), w.end());
    }
    for (const BigUint& s : ss) {
        w = s.to_limbs(sw);
        in.insert(in.end(), w.begin(), w.end());
    }
    for (const BigUint& c : res) {
        w = c.to_limbs(wr);
        in.insert(in.end(), w.begin(), w.end());
    }
    const std::vector<uint64_t>& tp = ctx.tape();
    std::vector<uint64_t> rec(K * per * 4 * wk, 0);
    for (size_t f = 0; f < K * per * 4; ++f) std::copy(tp.begin() + f * wr, tp.begin() + (f + 1) * wr, rec.begin() + f * wk);
    uint64_t* d_routes = d_work + rec.size();
    rc = pz_upload(ctx.raw(), d_work, rec.data(), rec.size() * 8);
    std::fill(rec.begin(), rec.end(), 0);
    if (rc == PZ_OK && !wit.routes.empty()) rc = pz_upload(ctx.raw(), d_routes, wit.routes.data(), wit.routes.size() * 8);
    if (rc == PZ_OK)
        rc = pz_smix_expand_dev(ctx.raw(), Ln, W, ctx.lookup_bits(), K, s_limbs, in.data(), wit.bits.empty() ? nullptr : wit.bits.data(),
                                layers ? d_routes : nullptr, d_work, d_modulus, d_advice, d_lookup, 0, 0);
    std::fill(in.begin(), in.end(), 0);
    return rc;
}

}  // namespace pz
