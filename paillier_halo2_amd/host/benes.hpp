// benes.hpp -- routing of the mix's switch network: host logic, no device code.
//
// The network over K = 2^d positions has 2d - 1 layers; layer l acts on bit beta(l) = l for l < d and 2d - 2 - l above.  Switch s of a
// layer is the s-th position j, ascending, with bit beta clear, its partner j | 2^beta; with bit b the switch leaves out[j] = b ? in[j']
// : in[j] and out[j'] = b ? in[j] : in[j'].  Values stay in place: the recursive Benes network whose outer layers pair neighbours and
// whose two inner networks live on the even and the odd positions.  Bits are layer-major, one byte each, (2d - 1) K / 2 in all.
//
// benes_route: the looping algorithm, level by level.  At level beta the 2^beta sub-networks (the positions sharing their low beta bits)
// are routed at once: every input is coloured with the inner network (bit beta of its next position) it travels through, such that the
// two inputs of a switch and the two inputs bound for the outputs of a switch take different ones; the colours are the level's input
// and output bits and give the inner networks' permutations.  perm[i] is the index of the input that output position i receives.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pz {

inline bool benes_is_count(size_t count) { return count >= 1 && count <= 1024 && (count & (count - 1)) == 0; }
inline unsigned benes_depth(size_t count) {
    unsigned d = 0;
    while (((size_t)1 << d) < count) ++d;
    return d;
}
inline size_t benes_layers(size_t count) { return count < 2 ? 0 : 2 * (size_t)benes_depth(count) - 1; }
// the index of the switch of a layer on bit beta that holds position j
inline size_t benes_switch(size_t j, unsigned beta) { return ((j >> (beta + 1)) << beta) | (j & (((size_t)1 << beta) - 1)); }

// false: count is not a power of two in 1 .. 1024, or perm is not a permutation of 0 .. count - 1 (bits is left as it was).
// The working arrays are overwritten before they are released: the permutation is a mixer's secret.
inline bool benes_route(size_t count, const uint32_t* perm, std::vector<uint8_t>& bits) {
    if (!benes_is_count(count) || !perm) return false;
    const size_t K = count, half = K / 2, none = ~(size_t)0;
    std::vector<size_t> P(K), inv(K, none), nextP(K);
    std::vector<uint8_t> sub(K), out(benes_layers(K) * half, 0);
    bool ok = true;
    for (size_t i = 0; i < K && ok; ++i) {
        if (perm[i] >= K || inv[perm[i]] != none) ok = false;
        else {
            P[i] = perm[i];
            inv[perm[i]] = i;
        }
    }
    const unsigned d = benes_depth(K);
    for (unsigned beta = 0; ok && beta + 1 < d; ++beta) {
        const size_t bit = (size_t)1 << beta;
        for (size_t i = 0; i < K; ++i) {
            inv[P[i]] = i;
            sub[i] = 2;   // not coloured yet
        }
        for (size_t o0 = 0; o0 < K; ++o0) {
            size_t o = o0;
            while (sub[P[o]] == 2) {
                const size_t a = P[o];
                sub[a] = 0;
                sub[a ^ bit] = 1;              // the other input of a's switch takes the other inner network,
                o = inv[a ^ bit] ^ bit;        // and so the other output of ITS output's switch is fed by this one again
            }
        }
        uint8_t* in_bits = out.data() + (size_t)beta * half;
        uint8_t* out_bits = out.data() + (size_t)(2 * d - 2 - beta) * half;
        for (size_t j = 0; j < K; ++j) {
            const size_t s = sub[P[j]], clear = ~bit;
            if (!(j & bit)) {
                in_bits[benes_switch(j, beta)] = sub[j];
                out_bits[benes_switch(j, beta)] = (uint8_t)s;
            }
            nextP[(j & clear) | (s << beta)] = (P[j] & clear) | (s << beta);
        }
        P.swap(nextP);
    }
    if (ok && d >= 1) {
        const size_t bit = (size_t)1 << (d - 1);
        uint8_t* mid = out.data() + (size_t)(d - 1) * half;
        for (size_t j = 0; j < K; ++j)
            if (!(j & bit)) mid[benes_switch(j, d - 1)] = P[j] != j;
    }
    if (ok) bits = out;
    auto wipe = [](volatile void* p, size_t n) {
        volatile unsigned char* c = (volatile unsigned char*)p;
        for (size_t i = 0; i < n; ++i) c[i] = 0;
    };
    wipe(P.data(), K * sizeof(size_t));
    wipe(inv.data(), K * sizeof(size_t));
    wipe(nextP.data(), K * sizeof(size_t));
    wipe(sub.data(), K);
    wipe(out.data(), out.size());
    return ok;
}

// every layer's outputs under `bits` (the reference for a device run): layers[l][position]
template <class V> inline std::vector<std::vector<V>> benes_apply(size_t count, const std::vector<uint8_t>& bits, const std::vector<V>& xs) {
    std::vector<std::vector<V>> layers;
    const unsigned d = benes_depth(count);
    const size_t n_layers = benes_layers(count), half = count / 2;
    std::vector<V> cur = xs;
    for (size_t l = 0; l < n_layers; ++l) {
        const unsigned beta = (unsigned)(l < d ? l : n_layers - 1 - l);
        std::vector<V> nxt = cur;
        for (size_t j = 0; j < count; ++j) {
            if (j & ((size_t)1 << beta)) continue;
            const size_t jp = j | ((size_t)1 << beta);
            if (bits[l * half + benes_switch(j, beta)]) {
                nxt[j] = cur[jp];
                nxt[jp] = cur[j];
            }
        }
        layers.push_back(nxt);
        cur = nxt;
    }
    return layers;
}

}   // namespace pz
