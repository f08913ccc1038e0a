"""The mix's switch network in Python integers: what csrc/pz_mix.cpp's pz_mix_route and the host mirror's
pz::benes_route compute, for callers that prepare a mixer's inputs without the library.  Host logic; no arithmetic on ciphertexts.

The network over K = 2^d positions has 2d - 1 layers.  Layer l acts on bit beta(l) = l for l < d and 2d - 2 - l above.  Switch s of a
layer is the s-th position j, ascending, with bit beta clear, its partner j' = j | 2^beta; with bit b it leaves out[j] = b ? in[j'] :
in[j] and out[j'] = b ? in[j] : in[j'].  Values stay in place.  Bits are layer-major, one byte each, (2d - 1) K / 2 in all.  perm[i] is
the index of the input that output position i receives."""
from __future__ import annotations

import secrets
from typing import Callable, List, Sequence

MIX_MAX = 1024      # ciphertexts of one mix (pz.h pz_paillier_mix)


def is_count(count: int) -> bool:
    return isinstance(count, int) and 1 <= count <= MIX_MAX and count & (count - 1) == 0


def depth(count: int) -> int:
    if not is_count(count):
        raise ValueError(f"a mix takes count = 1, 2, 4 .. {MIX_MAX} ciphertexts, not {count}")
    return count.bit_length() - 1


def layer_bits(count: int) -> List[int]:
    """beta(l) for l = 0 .. 2d - 2: 0, 1, .., d - 1, .., 1, 0 (empty for count = 1)"""
    d = depth(count)
    return [l if l < d else 2 * d - 2 - l for l in range(2 * d - 1)] if d else []


def switch_index(j: int, beta: int) -> int:
    """the index of the switch of a layer on bit beta that holds position j"""
    return ((j >> (beta + 1)) << beta) | (j & ((1 << beta) - 1))


def benes_route(perm: Sequence[int]) -> bytes:
    """the switch bits under which output position i receives input perm[i]: the looping algorithm, level by level.  At level beta the
    positions that share their low beta bits form one sub-network; every input is coloured with the inner network it travels through
    (bit beta of its next position), such that the two inputs of a switch, and the two inputs bound for the two outputs of a switch,
    take different ones.  The colours are the level's input and output bits and give the inner networks' permutations."""
    K = len(perm)
    d = depth(K)
    P = [int(p) for p in perm]
    if sorted(P) != list(range(K)):
        raise ValueError("perm is not a permutation of 0 .. count - 1")
    half = K // 2
    out = bytearray((2 * d - 1) * half if d else 0)
    for beta in range(d - 1):
        bit = 1 << beta
        inv = [0] * K
        for i, p in enumerate(P):
            inv[p] = i
        sub = [2] * K
        for o0 in range(K):
            o = o0
            while sub[P[o]] == 2:
                a = P[o]
                sub[a], sub[a ^ bit] = 0, 1     # the other input of a's switch takes the other inner network,
                o = inv[a ^ bit] ^ bit          # and so the other output of ITS output's switch is fed by this one again
        nxt = [0] * K
        lo, hi = beta * half, (2 * d - 2 - beta) * half
        for j in range(K):
            s = sub[P[j]]
            if not j & bit:
                out[lo + switch_index(j, beta)] = sub[j]
                out[hi + switch_index(j, beta)] = s
            nxt[(j & ~bit) | (s << beta)] = (P[j] & ~bit) | (s << beta)
        P = nxt
    if d:
        bit = 1 << (d - 1)
        for j in range(K):
            if not j & bit:
                out[(d - 1) * half + switch_index(j, d - 1)] = int(P[j] != j)
    return bytes(out)


def benes_apply(bits: Sequence[int], xs: Sequence) -> list:
    """the network's outputs for the inputs xs under `bits` (each 0 or 1): a permutation of xs whatever the bits are"""
    K = len(xs)
    half = K // 2
    betas = layer_bits(K)
    if len(bits) != len(betas) * half:
        raise ValueError(f"{K} positions take {len(betas) * half} switch bits, not {len(bits)}")
    if any(b not in (0, 1) for b in bits):
        raise ValueError("a switch bit is 0 or 1")
    cur = list(xs)
    for l, beta in enumerate(betas):
        for j in range(K):
            if not j & (1 << beta) and bits[l * half + switch_index(j, beta)]:
                jp = j | (1 << beta)
                cur[j], cur[jp] = cur[jp], cur[j]
    return cur


def random_permutation(count: int, rand: Callable[[int], int] = secrets.randbelow) -> List[int]:
    """a uniform permutation of 0 .. count - 1 (Fisher-Yates over rand(k), uniform below k: the system's generator by default)"""
    perm = list(range(count))
    for i in range(count - 1, 0, -1):
        j = rand(i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    return perm
