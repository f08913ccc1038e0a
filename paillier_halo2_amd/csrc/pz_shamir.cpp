// pz_shamir.cpp -- the Lagrange exponents of a t-of-T threshold decryption as an entry point: host logic only,
// no context, no kernel.  For the member ids S of a combination (distinct, 1 .. trustees) the exponent of member i is
//   mu_i = trustees! * prod_{j in S, j != i} j / (j - i),
// an integer (Shoup, "Practical threshold signatures", Eurocrypt 2000, section 2.1), computed exactly here over host/biguint.hpp --
// trustees! times the other ids, then one exact division per difference -- and handed out as a magnitude and a sign byte: what
// pz_paillier_combine_t takes.  A remainder in any of the divisions would contradict the integrality and is reported as PZ_ERR_INTERNAL.
#include <cstring>
#include <vector>

#include "../../include/pz.h"
#include "../host/biguint.hpp"

extern "C" int pz_shamir_lagrange(uint32_t trustees, size_t members, const uint32_t* ids, uint64_t* exps_out, uint32_t exp_words,
                                  uint8_t* neg_out, uint32_t* words_needed) {
    if (!ids || !exps_out || !neg_out || exp_words == 0) return PZ_ERR_INVALID;
    if (trustees < 1 || trustees > 256 || members < 1 || members > trustees) return PZ_ERR_INVALID;
    bool seen[257] = {false};
    for (size_t k = 0; k < members; ++k) {
        if (ids[k] < 1 || ids[k] > trustees || seen[ids[k]]) return PZ_ERR_INVALID;
        seen[ids[k]] = true;
    }
    try {
        pz::BigUint delta(1);
        for (uint32_t f = 2; f <= trustees; ++f) delta = delta.mul_small(f);
        std::vector<pz::BigUint> mu(members);
        size_t need = 1;
        for (size_t k = 0; k < members; ++k) {
            const uint32_t i = ids[k];
            pz::BigUint num = delta;
            unsigned below = 0;
            for (size_t t = 0; t < members; ++t)
                if (t != k) num = num.mul_small(ids[t]);
            for (size_t t = 0; t < members; ++t) {
                if (t == k) continue;
                const uint32_t j = ids[t];
                uint64_t rem = 0;
                num = num.divmod_small(j > i ? j - i : i - j, rem);
                if (rem) return PZ_ERR_INTERNAL;
                below += j < i;
            }
            if (num.is_zero()) return PZ_ERR_INTERNAL;
            neg_out[k] = (uint8_t)(below & 1);
            need = num.l.size() > need ? num.l.size() : need;
            mu[k] = num;
        }
        if (words_needed) *words_needed = (uint32_t)need;
        if (need > exp_words) return PZ_ERR_CAPACITY;
        for (size_t k = 0; k < members; ++k) {
            const std::vector<uint64_t> w = mu[k].to_limbs(exp_words);
            std::memcpy(exps_out + k * exp_words, w.data(), (size_t)exp_words * 8);
        }
    } catch (const std::exception&) {
        return PZ_ERR_INTERNAL;
    }
    return PZ_OK;
}
