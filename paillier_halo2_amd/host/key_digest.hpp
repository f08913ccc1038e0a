// key_digest.hpp -- the verifying key's digest, the ONE definition behind pz_key_digest / pz_pk_digest / pz_vk_digest (csrc/) and the compiled
// drivers (prove_connected.cpp): what a bound Fiat-Shamir transcript starts from, where halo2 absorbs vk.transcript_repr (DESIGN.md
// section 15.6).  prover.py::key_digest states the same function with hashlib.
//   D = BLAKE2b-512, personalised "PZ-Key-Digest-v1", over
//       six little-endian u64: k, blinding_factors, n_adv, n_lk, n_instance, n_public
//       fixed_affine: (n_adv + 2) x 8 words | sigma_affine: (n_adv + n_lk + 1 + n_instance) x 8 words
// both arrays exactly as pz_pk_commitments / pz_vk_keygen* / pz_vk_create[_pub] carry them (Montgomery words, little-endian: the form the
// transcript absorbs points in).  lookup_bits is pinned by the table column's commitment; the params are not part of it (nor of halo2's).
// A bound transcript is the unbound one with D || seed for its seed bytes: nothing after the seed moves.
#pragma once
#include <cstddef>
#include <cstdint>

#include "blake2b.hpp"

namespace pzh {

constexpr size_t KEY_DIGEST_BYTES = 64;

inline void key_digest(uint64_t k, uint64_t blinding_factors, uint64_t n_adv, uint64_t n_lk, uint64_t n_instance, uint64_t n_public,
                       const uint64_t* fixed_affine, const uint64_t* sigma_affine, uint8_t out[KEY_DIGEST_BYTES]) {
    Blake2b h("PZ-Key-Digest-v1");
    const uint64_t shape[6] = {k, blinding_factors, n_adv, n_lk, n_instance, n_public};
    h.update(shape, sizeof shape);
    h.update(fixed_affine, 64 * (size_t)(n_adv + 2));
    h.update(sigma_affine, 64 * (size_t)(n_adv + n_lk + 1 + n_instance));
    h.digest(out);
}

}   // namespace pzh
