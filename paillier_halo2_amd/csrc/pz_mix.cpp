// pz_mix.cpp -- the switch bits of a mixer's permutation as an entry point: host logic only, no context, no
// kernel.  perm[i] is the index of the input that output position i receives; bits_out takes the (2 log2(count) - 1) * count / 2 bytes
// of the Benes network that pz_paillier_mix applies, layer-major (../host/benes.hpp: the looping algorithm, shared with the host
// mirror).  The permutation is the mixer's secret: the routine keeps nothing of it once it has returned.
#include <cstring>
#include <exception>
#include <vector>

#include "../../include/pz.h"
#include "../host/benes.hpp"

extern "C" int pz_mix_route(size_t count, const uint32_t* perm, uint8_t* bits_out) {
    if (!perm || !pz::benes_is_count(count) || (!bits_out && count > 1)) return PZ_ERR_INVALID;
    try {
        std::vector<uint8_t> bits;
        if (!pz::benes_route(count, perm, bits)) return PZ_ERR_INVALID;
        if (!bits.empty()) {
            std::memcpy(bits_out, bits.data(), bits.size());
            volatile uint8_t* w = bits.data();
            for (size_t i = 0; i < bits.size(); ++i) w[i] = 0;
        }
    } catch (const std::exception&) {
        return PZ_ERR_INTERNAL;
    }
    return PZ_OK;
}
