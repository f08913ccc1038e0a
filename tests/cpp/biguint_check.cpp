// biguint_check.cpp -- host/biguint.hpp operation by operation, for tests/test_cpp_biguint.py to hold to Python integers.
// Reads lines `op hex hex [hex|int]` from stdin (an operation with one operand takes a second one it ignores), prints one line per
// input line: the result in hex (two for divmod and divmod_small), or `throw:<type>`.
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../paillier_halo2_amd/host/biguint.hpp"

using pz::BigUint;

static std::string run(const std::string& op, const BigUint& a, const BigUint& b, const std::string& third) {
    const size_t k = third.empty() ? 0 : (size_t)std::strtoull(third.c_str(), nullptr, 10);
    if (op == "add") return (a + b).to_hex();
    if (op == "sub") return (a - b).to_hex();
    if (op == "mul") return (a * b).to_hex();
    if (op == "shl") return (a << k).to_hex();
    if (op == "shr") return (a >> k).to_hex();
    if (op == "low_bits") return a.low_bits(k).to_hex();
    if (op == "divmod") {
        BigUint q, r;
        BigUint::divmod(a, b, q, r);
        return q.to_hex() + " " + r.to_hex() + " " + (a / b).to_hex() + " " + (a % b).to_hex();
    }
    if (op == "mul_small") return a.mul_small(b.l.empty() ? 0 : b.l[0]).to_hex();
    if (op == "divmod_small") {
        uint64_t rem = 0;
        const BigUint q = a.divmod_small(b.l.empty() ? 0 : b.l[0], rem);
        return q.to_hex() + " " + BigUint(rem).to_hex();
    }
    if (op == "reduce_near") return BigUint::reduce_near(a, b, (unsigned)k).to_hex();
    if (op == "gcd") return BigUint::gcd(a, b).to_hex();
    if (op == "mod_inverse") return BigUint::mod_inverse(a, b).to_hex();
    if (op == "lt") return std::string(a < b ? "1" : "0") + (a == b ? " 1" : " 0") + (a != b ? " 1" : " 0");
    if (op == "bits") {
        std::ostringstream o;
        o << a.bits() << " " << (a.is_zero() ? 1 : 0) << " " << (a.bit(k) ? 1 : 0) << " " << a.l.size();
        return o.str();
    }
    if (op == "hex") return a.to_hex();
    if (op == "limbs") {   // to_limbs(k) and back through from_limbs: throws if the value does not fit k limbs
        const std::vector<uint64_t> w = a.to_limbs(k);
        return BigUint::from_limbs(w.data(), w.size()).to_hex();
    }
    throw std::invalid_argument("op");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, ha, hb, third;
        in >> op >> ha >> hb >> third;
        if (op.empty()) continue;
        try {
            std::cout << run(op, BigUint::from_hex(ha), BigUint::from_hex(hb), third) << "\n";
        } catch (const std::range_error&) {
            std::cout << "throw:range_error\n";
        } catch (const std::domain_error&) {
            std::cout << "throw:domain_error\n";
        } catch (const std::invalid_argument&) {
            std::cout << "throw:invalid_argument\n";
        }
    }
    return 0;
}
