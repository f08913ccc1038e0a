"""halo2's KZG / SHPLONK verifier for the proofs of this package, without the toxic scalar: the last step is a pairing check on the device.

Per proof (what halo2-axiom's `verify_proof` does for these circuits [D]):
  1. replay the Fiat-Shamir transcript (prover.HashTranscript's function) from the seed and the proof's own commitments and
     evaluations: theta, beta, gamma, y, x, SHPLONK's y, v, u.  Nothing the prover recorded about its challenges is read.
  2. h(x) (x^n - 1) == the constraint expression of the evaluations: the gates q (a + b c - d), the chunked permutation argument (delta
     powers) and the lookups, restated here from the evaluations alone.
  3. the h commitment sum_i x^(n i) [h_i] (three pieces).
  4. SHPLONK's G1 terms A = L + z_0 u W2, B = -z_0 W2 with L = sum_k v^k z_k (sum_j y^j C_kj - [R_k(u)]) - Z_T(u) W1; the proof holds
     iff e(A, [1]_2) e(B, [s]_2) == 1.

verify_batch folds B proofs with random r_i (os.urandom) into sum r_i A_i, sum r_i B_i: ONE device MSM (K1, two scalar columns) over the
key's fixed and sigma commitments (once, their scalars summed over the proofs), the generator and every proof's own commitments, then ONE
2-pair pz_pairing_check_dev.  If that fails, or an identity of step 2 fails, the per-proof verdicts come from B independent checks in
one pz_pairing_check_dev launch.  A proof with a commitment that is off the curve or has a coordinate that is not canonical (the identity
(0, 0) apart), or with an evaluation >= r, is False by itself and takes no part in the rest.  The transcript seed is the caller's bytes;
with bind_key=True every verifier here replays from VerifyingKey.digest() + seed instead: the proof must have
been made with HashTranscript(seed, key_digest=...) of the SAME key, and a proof made without it is False.
"""
from __future__ import annotations

import hashlib
import os
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import consts
from .prover import CHUNK, DELTA, Domain, key_digest, query_layout, rotation_points

R = consts.FR_R
H_PIECES = 3
COMMITMENT_ROUNDS = ((("advice", "lookup_advice"), ("theta",)), (("perm_inputs", "perm_tables"), ("beta", "gamma")),
                     (("perm_z", "lookup_z", "random"), ("y",)), (("h",), ("x",)))
EVAL_FAMILIES = ("advice", "lookup_advice", "fixed", "sigma", "perm_z", "lookup_z", "perm_inputs", "perm_tables", "random")
_MONT_INV = pow(consts.MONT_R, -1, R)
_MONT_INV_Q = pow(consts.MONT_R, -1, consts.FQ_P)


@dataclass
class VerifierParams:
    """the verifier's side of ParamsKZG: g[0] (8 words), g2 and s_g2 (16 words each, Montgomery)"""
    g0: np.ndarray
    g2: np.ndarray
    s_g2: np.ndarray

    @classmethod
    def from_parts(cls, g0, g2, s_g2) -> "VerifierParams":
        w = lambda b: np.frombuffer(bytes(b), dtype="<u8").astype(np.uint64) if isinstance(b, (bytes, bytearray)) else \
            np.ascontiguousarray(b, dtype=np.uint64).reshape(16)
        p = cls(np.ascontiguousarray(g0, dtype=np.uint64).reshape(8), w(g2), w(s_g2))
        if p.g2.shape != (16,) or p.s_g2.shape != (16,):
            raise ValueError("g2 / s_g2 must be 16 words (128 RawBytes) each")
        if not p.g2.any() or not p.s_g2.any():
            raise ValueError("the params carry no G2 elements (g2 / s_g2 are zero): no KZG proof can be checked against them")
        if not p.g0.any():
            raise ValueError("g[0] is the identity")
        return p

    @classmethod
    def from_params(cls, params) -> "VerifierParams":
        """from srs.ParamsKZG (read_params_kzg)"""
        return cls.from_parts(np.asarray(params.g[0]), params.g2, params.s_g2)


@dataclass
class VerifyingKey:
    """the circuit's shape and the key's commitments (ProvingKey.vk_commitments(): fixed [n_adv + 2], sigma [m], affine)"""
    k: int
    blinding_factors: int
    n_adv: int
    n_lk: int
    n_sets: int
    fixed: np.ndarray
    sigma: np.ndarray
    n_instance: int = 0            # 1: the key's permutation ends with the instance column (public inputs)
    n_public: int = 0              # values of the statement

    @property
    def m(self) -> int:
        return self.n_adv + self.n_lk + 1 + self.n_instance

    def digest(self) -> bytes:
        """the key's 64-byte digest (prover.key_digest; equal to pz_pk_digest / pz_vk_digest of the same key): what a bound transcript starts
        from.  Computable from a PZVK file's contents alone"""
        return key_digest(self.k, self.blinding_factors, self.n_adv, self.n_lk, self.fixed, self.sigma, self.n_instance, self.n_public)

    @classmethod
    def from_proving_key(cls, pk) -> "VerifyingKey":
        vk = pk.vk_commitments()
        st = pk.st
        return cls(st.k, st.blinding_factors, st.n_adv, st.n_lk, pk.n_sets, vk["fixed"], vk["sigma"], getattr(st, "n_instance", 0),
                   getattr(st, "n_public", 0))


    @classmethod
    def from_structure(cls, eng, st, bases_lagrange, tile: int = 64) -> "VerifyingKey":
        """keygen_vk: the key from the circuit STRUCTURE alone (pz_vk_keygen[_dev]; no proving key is built, device memory O(tile 2^k)) --
        the same object from_proving_key returns for a key made from `st`.  st: a CircuitStructure whose selectors / map_col / map_row
        are torch tensors on the device (used where they are) or numpy arrays (uploaded tile by tile), or a NativeStructure (the device
        arrays of a pz_circuit_structure_dev handle)."""
        k, A, Lk = st.k, st.n_adv, st.n_lk
        ni, npub = getattr(st, "n_instance", 0), getattr(st, "n_public", 0)
        if hasattr(st, "d_selectors"):                      # a pz_structure handle's arrays
            fixed, sigma = eng.vk_keygen_dev(bases_lagrange, k, st.lookup_bits, A, Lk, st.d_selectors, st.constants(), st.d_map_col,
                                             st.d_map_row, tile, ni, npub)
        else:
            if getattr(st, "table", None) is not None:
                raise ValueError("keygen_vk commits the table 0 .. 2^lookup_bits - 1; this structure carries another one")
            consts_ = [int(v) % R for v in st.constants]
            if hasattr(st.selectors, "is_cuda"):
                import torch

                sel = st.selectors.cuda().to(torch.uint8).contiguous()
                mc, mr = st.map_col.cuda().to(torch.int32).contiguous(), st.map_row.cuda().to(torch.int32).contiguous()
                if tuple(sel.shape) != (A, 1 << k) or tuple(mc.shape) != (A + Lk + 1 + ni, 1 << k) or mc.shape != mr.shape:
                    raise ValueError("selectors must be [n_adv][2^k], map_col / map_row [m][2^k]")
                torch.cuda.current_stream().synchronize()   # the conversions above may have run on another stream than the library's
                fixed, sigma = eng.vk_keygen_dev(bases_lagrange, k, st.lookup_bits, A, Lk, sel.data_ptr(), consts_, mc.data_ptr(), mr.data_ptr(),
                                                 tile, ni, npub)
            else:
                fixed, sigma = eng.vk_keygen(bases_lagrange, k, st.lookup_bits, A, Lk, st.selectors, consts_, st.map_col, st.map_row, tile, ni, npub)
        return cls(k, st.blinding_factors, A, Lk, -(-(A + Lk + 1 + ni) // CHUNK), fixed, sigma, ni, npub)


def _ints(a) -> List[List[int]]:
    """(count, points, 4) Montgomery words -> canonical integers [[..]]"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    rows = a.reshape(a.shape[0], -1, 4)
    out = []
    for row in rows:
        vals = []
        for w in row:
            v = int(w[0]) | int(w[1]) << 64 | int(w[2]) << 128 | int(w[3]) << 192
            vals.append(v * _MONT_INV % R)
        out.append(vals)
    return out


def _points_ok(a) -> bool:
    """pz_g1_check_dev's rule for every row of (count, 8) Montgomery words: the identity (0, 0), or canonical coordinates (below p) of a
    point on y^2 = x^3 + 3 -- what the wire decoder and halo2's `read` ask of a commitment"""
    p = consts.FQ_P
    for row in np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 8):
        xm, ym = consts.limbs_to_int(row[:4]), consts.limbs_to_int(row[4:])
        if xm == 0 and ym == 0:
            continue
        if xm >= p or ym >= p:
            return False
        x, y = xm * _MONT_INV_Q % p, ym * _MONT_INV_Q % p
        if (y * y - x * x * x - 3) % p:
            return False
    return True


def _evals_canonical(a) -> bool:
    """every evaluation's Montgomery words are below r"""
    return all(consts.limbs_to_int(w) < R for w in np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4))


def proof_from_record(rec: Dict[str, np.ndarray], prefix: str, vk: VerifyingKey):
    """proof `prefix` ("p0/", ...) of a prover_job.read_proofs record -> (commitments, evals) in prover.Proof's shapes (the record's
    lookup-advice evaluations carry the constants row last)"""
    com = {k[len(prefix) + 2:]: np.asarray(v, dtype=np.uint64).reshape(-1, 8) for k, v in rec.items() if k.startswith(prefix + "c/")}
    ev = {k[len(prefix) + 2:]: np.asarray(v, dtype=np.uint64).reshape(v.shape[0], -1, 4) for k, v in rec.items()
          if k.startswith(prefix + "e/")}
    if "lookup_advice" in ev:
        ev["constants"] = ev["lookup_advice"][vk.n_lk:]
        ev["lookup_advice"] = ev["lookup_advice"][:vk.n_lk]
    return com, ev


def record_seed(prefix: str) -> bytes:
    """the compiled prover seeds proof `prefix` ("p<i>/")'s transcript with i as 8 little-endian bytes"""
    return int(prefix[1:-1]).to_bytes(8, "little")


def public_inputs(kind: str, n: int, g: Optional[int] = None, c: Optional[int] = None, c1: Optional[int] = None, c2: Optional[int] = None, *,
                  enc_bits: int, limb_bits: int, cts: Optional[Sequence[int]] = None, weights: Optional[Sequence[int]] = None,
                  m: Optional[int] = None, total: Optional[int] = None, v: Optional[int] = None, h: Optional[int] = None,
                  partials: Optional[Sequence[int]] = None, mixed: Optional[Sequence[int]] = None, hs: Optional[int] = None,
                  slots: Optional[int] = None, slot_bits: Optional[int] = None, m_bits: Optional[int] = None,
                  totals: Optional[Sequence[int]] = None) -> List[int]:
    """the statement of a circuit with the instance column, in the column's row order: little-endian limbs of limb_bits,
    n | g | c (kind "encrypt" / "encrypt_uniform": c = g^m r^n mod n^2) or n | g | c1 | c2 | c ("add": c = c1 c2 mod n^2); n, g, c1, c2 have
    enc_bits / limb_bits limbs, c twice as many.  (The add circuit's c1 and c2 are its enc_bits-wide inputs x and y.)
    kind "tally": n | c_1 | .. | c_B | c with cts = [c_1 .. c_B] at full width (twice n's limbs each) and c their product mod n^2; g plays
    no part in an addition and is ignored.
    kind "wtally": n | c_1 | .. | c_B | w_1 | .. | w_B | c with c = prod c_i^w_i mod n^2, B >= 1; a weight is ONE value (one cell of
    the circuit, below 2^64), not limbs.
    kind "decrypt": n | g | m | c -- "c decrypts to m under (n, g)", i.e. there is an r with c = g^m r^n mod n^2.  The circuit does not
    compare m with n: the verifier does, HERE (both are public), and an m >= n is refused -- with it the statement says nothing
    about Dec(c).
    kind "ballot": n | g | c_1 | .. | c_K | S -- "every c_i of cts encrypts a value below 2^m_bits under (n, g), and the values add up to
    S = total"; m_bits is the circuit's shape, not part of the statement.  One ciphertext has no S (it would be the message): a total
    given with K = 1 is refused, and so is a total missing with K >= 2.  S is ONE value.  A c_i >= n^2 is no ciphertext and is refused
    here (the circuit proves c_i = a remainder mod n^2, so no proof exists for one).  No single result c.
    kind "partial": n | v | h | c_1 | u_1 | .. | c_K | u_K -- "the trustee whose public share is h = v^theta opened every c_j of cts to
    u_j = (c_j^2)^theta mod n^2 (partials) with that one theta"; v and h come from the public threshold key (keys.ThresholdKey.v, .hs[i]).
    The circuit compares nothing with n^2: the verifier does, HERE, and a v, h, c_j or u_j >= n^2 is refused, as are cts and partials of
    different lengths.  No g and no single result c.
    kind "mix": n | c_1 | .. | c_K | c'_1 | .. | c'_K -- "the list mixed is a re-randomised permutation of the list cts under the key
    n": there are a permutation pi and r_i with c'_i = c_pi(i) r_i^n mod n^2.  K is a power of two (1 .. 1024); lists of different
    lengths are refused, and so is any c_j or c'_i >= n^2 (no ciphertext) and any c'_i = 0 -- what a mixer's r_i = 0 leaves: a vote
    destroyed in plain sight, which the circuit does not exclude (any other non-unit output needs a factor of n).  No g and no
    single result c.
    kind "sballot": n | g | hs | c_1 | .. | c_K | S -- "every c_i of cts is g^m_i hs^s_i mod n^2 with m_i below 2^m_bits and s_i below
    2^s_bits, and the m_i add up to S = total"; hs = h^n mod n^2 is the key's (keys.djn_generator), m_bits and s_bits are the circuit's
    shape.  total as in "ballot": refused with K = 1, required with K >= 2.  hs = 0 (every c_i would be 0), an hs >= n^2 and a c_i >=
    n^2 are refused here: the circuit compares nothing with n^2.  That hs is an n-th residue is the key authority's to show, not this
    statement's.
    kind "smix": n | hs | c_1 | .. | c_K | c'_1 | .. | c'_K -- "the list mixed is a re-randomised permutation of the list cts under the
    key (n, hs)": there are a permutation pi and s_i below 2^s_bits with c'_i = c_pi(i) hs^s_i mod n^2.  K is a power of two (1 ..
    1024); lists of different lengths are refused, and so are hs = 0 (every output would be 0), an hs >= n^2, any c_j or c'_i >= n^2 and
    any c'_i = 0.  No g and no single result c.  c'_i holds what c_pi(i) holds only if hs is an n-th residue: that is the key
    authority's to show, not this statement's.
    kind "pballot": n | hs | G_0 | .. | G_{K-1} | c_1 | .. | c_R | S_1 | .. | S_R -- "every c_i of cts is (prod_j G_j^v_ij) hs^s_i mod n^2
    with every v_ij below 2^m_bits, s_i below 2^s_bits and sum_j v_ij = S_i = totals[i]", i.e. c_i = g^M_i hs^s_i with the packed
    plaintext M_i = sum_j v_ij 2^(j w), K = slots, w = slot_bits.  The slot bases G_j = g^(2^(j w)) mod n^2 are DERIVED HERE from (n, g,
    K, w) in Python integers: a statement cannot name bases of its own.  Refused: 2^(K w) > n (a packed plaintext would wrap), m_bits >
    slot_bits (a slot value would reach into the next slot), hs = 0, an hs >= n^2, any c_i >= n^2, totals given with K = 1, totals
    missing with K >= 2 or of another length than cts.  Each S_i is ONE field value.  No single result c; that hs is an n-th residue
    is the key authority's to show."""
    Ln = enc_bits // limb_bits
    mask = (1 << limb_bits) - 1
    limbs = lambda v, cnt: [(int(v) >> (limb_bits * i)) & mask for i in range(cnt)]
    if kind == "add":
        if c1 is None or c2 is None:
            raise ValueError("the add statement names both ciphertexts c1 and c2")
        parts = [(n, Ln), (g, Ln), (c1, Ln), (c2, Ln), (c, 2 * Ln)]
    elif kind in ("encrypt", "encrypt_uniform"):
        parts = [(n, Ln), (g, Ln), (c, 2 * Ln)]
    elif kind == "decrypt":
        if m is None:
            raise ValueError("the decrypt statement names the plaintext m")
        if not 0 <= int(m) < int(n):
            raise ValueError("the decrypt statement needs 0 <= m < n")
        parts = [(n, Ln), (g, Ln), (m, Ln), (c, 2 * Ln)]
    elif kind == "tally":
        if cts is None or len(cts) < 2:
            raise ValueError("the tally statement names its ciphertexts: cts = [c_1 .. c_B], B >= 2")
        parts = [(n, Ln)] + [(ci, 2 * Ln) for ci in cts] + [(c, 2 * Ln)]
    elif kind == "wtally":
        if cts is None or weights is None or len(cts) < 1 or len(weights) != len(cts):
            raise ValueError("the weighted tally's statement names its ciphertexts and one weight each: cts = [c_1 .. c_B], weights = [w_1 .. w_B]")
        if any(int(v) < 0 or int(v) >> 64 for v in weights):
            raise ValueError("a weight does not fit 64 bits")
        parts = [(n, Ln)] + [(ci, 2 * Ln) for ci in cts] + [(c, 2 * Ln)]
    elif kind == "ballot":
        if cts is None or len(cts) < 1 or g is None or c is not None:
            raise ValueError("the ballot statement names n, g and its ciphertexts cts = [c_1 .. c_K], K >= 1, and no single result c")
        if (total is not None) != (len(cts) >= 2):
            raise ValueError("the ballot statement carries the sum `total` exactly when it has two or more ciphertexts")
        if total is not None and (int(total) < 0 or int(total) >= consts.FR_R):
            raise ValueError("the total is one field value")
        if any(int(ci) >= int(n) * int(n) for ci in cts):
            raise ValueError("a ballot's ciphertext is below n^2")
        parts = [(n, Ln), (g, Ln)] + [(ci, 2 * Ln) for ci in cts]
    elif kind == "sballot":
        if cts is None or len(cts) < 1 or g is None or hs is None or c is not None:
            raise ValueError("the sballot statement names n, g, hs and its ciphertexts cts = [c_1 .. c_K], K >= 1, and no single result c")
        if (total is not None) != (len(cts) >= 2):
            raise ValueError("the sballot statement carries the sum `total` exactly when it has two or more ciphertexts")
        if total is not None and (int(total) < 0 or int(total) >= consts.FR_R):
            raise ValueError("the total is one field value")
        if not 0 < int(hs) < int(n) * int(n):
            raise ValueError("hs is neither 0 nor n^2 or more")
        if any(not 0 <= int(ci) < int(n) * int(n) for ci in cts):
            raise ValueError("a ballot's ciphertext is below n^2")
        parts = [(n, Ln), (g, Ln), (hs, 2 * Ln)] + [(ci, 2 * Ln) for ci in cts]
    elif kind == "partial":
        if v is None or h is None or cts is None or partials is None or len(cts) < 1 or g is not None or c is not None:
            raise ValueError("the partial statement names n, v, h, cts = [c_1 .. c_K] and partials = [u_1 .. u_K], K >= 1, and neither g nor c")
        if len(partials) != len(cts):
            raise ValueError("the partial statement has one partial decryption per ciphertext")
        if any(not 0 <= int(x) < int(n) * int(n) for x in [v, h] + list(cts) + list(partials)):
            raise ValueError("v, h, every ciphertext and every partial decryption are below n^2")
        parts = [(n, Ln), (v, 2 * Ln), (h, 2 * Ln)]
        for ci, ui in zip(cts, partials):
            parts += [(ci, 2 * Ln), (ui, 2 * Ln)]
    elif kind == "mix":
        if cts is None or mixed is None or g is not None or c is not None:
            raise ValueError("the mix statement names n, cts = [c_1 .. c_K] and mixed = [c'_1 .. c'_K], and neither g nor c")
        if len(mixed) != len(cts):
            raise ValueError("the mix statement has one output per input")
        if not (1 <= len(cts) <= 1024 and len(cts) & (len(cts) - 1) == 0):
            raise ValueError("a mix takes 1, 2, 4 .. 1024 ciphertexts")
        if any(not 0 <= int(x) < int(n) * int(n) for x in list(cts) + list(mixed)):
            raise ValueError("every input and every output of a mix is below n^2")
        if any(int(x) == 0 for x in mixed):
            raise ValueError("an output of a mix is not 0: a mixer's r_i = 0 destroys the ciphertext")
        parts = [(n, Ln)] + [(ci, 2 * Ln) for ci in cts] + [(ci, 2 * Ln) for ci in mixed]
    elif kind == "smix":
        if cts is None or mixed is None or hs is None or g is not None or c is not None:
            raise ValueError("the smix statement names n, hs, cts = [c_1 .. c_K] and mixed = [c'_1 .. c'_K], and neither g nor c")
        if len(mixed) != len(cts):
            raise ValueError("the smix statement has one output per input")
        if not (1 <= len(cts) <= 1024 and len(cts) & (len(cts) - 1) == 0):
            raise ValueError("a mix takes 1, 2, 4 .. 1024 ciphertexts")
        if not 0 < int(hs) < int(n) * int(n):
            raise ValueError("hs is neither 0 nor n^2 or more")
        if any(not 0 <= int(x) < int(n) * int(n) for x in list(cts) + list(mixed)):
            raise ValueError("every input and every output of a mix is below n^2")
        if any(int(x) == 0 for x in mixed):
            raise ValueError("an output of a mix is not 0")
        parts = [(n, Ln), (hs, 2 * Ln)] + [(ci, 2 * Ln) for ci in cts] + [(ci, 2 * Ln) for ci in mixed]
    elif kind == "pballot":
        if cts is None or len(cts) < 1 or g is None or hs is None or c is not None or total is not None:
            raise ValueError("the pballot statement names n, g, hs and its ciphertexts cts = [c_1 .. c_R], R >= 1, and neither c nor total")
        for x in (slots, slot_bits, m_bits):
            if x is None or isinstance(x, bool) or not isinstance(x, int) or x < 1:
                raise ValueError("the pballot statement names slots, slot_bits and m_bits, positive integers")
        if (1 << (slots * slot_bits)) > int(n):
            raise ValueError("the packed plaintext of slots * slot_bits bits must stay below n")
        if m_bits > slot_bits:
            raise ValueError("a slot value of m_bits bits does not fit a slot of slot_bits bits")
        if not 0 < int(hs) < int(n) * int(n):
            raise ValueError("hs is neither 0 nor n^2 or more")
        if any(not 0 <= int(ci) < int(n) * int(n) for ci in cts):
            raise ValueError("a ballot's ciphertext is below n^2")
        if (totals is not None) != (slots >= 2):
            raise ValueError("the pballot statement carries the sums `totals` exactly when it has two or more slots")
        if totals is not None and len(totals) != len(cts):
            raise ValueError("the pballot statement has one total per ciphertext")
        if totals is not None and any(int(t) < 0 or int(t) >= consts.FR_R for t in totals):
            raise ValueError("a total is one field value")
        n2 = int(n) * int(n)
        parts = [(n, Ln), (hs, 2 * Ln)] + [(pow(int(g), 1 << (j * slot_bits), n2), 2 * Ln) for j in range(slots)]
        parts += [(ci, 2 * Ln) for ci in cts]
    else:
        raise ValueError("kind must be encrypt, add, encrypt_uniform, tally, wtally, decrypt, ballot, partial, mix, sballot, smix or pballot")
    if (slots is not None or slot_bits is not None or m_bits is not None or totals is not None) and kind != "pballot":
        raise ValueError("slots, slot_bits, m_bits and totals belong to kind 'pballot'")
    if hs is not None and kind not in ("sballot", "smix", "pballot"):
        raise ValueError("hs belongs to kinds 'sballot', 'smix' and 'pballot'")
    if mixed is not None and kind not in ("mix", "smix"):
        raise ValueError("mixed belongs to kinds 'mix' and 'smix'")
    if c is None and kind not in ("ballot", "partial", "mix", "sballot", "smix", "pballot"):
        raise ValueError("the statement names its result c")
    if (v is not None or h is not None or partials is not None) and kind != "partial":
        raise ValueError("v, h and partials belong to kind 'partial'")
    if total is not None and kind not in ("ballot", "sballot"):
        raise ValueError("total belongs to kinds 'ballot' and 'sballot'")
    if m is not None and kind != "decrypt":
        raise ValueError("m belongs to kind 'decrypt'")
    if cts is not None and kind not in ("tally", "wtally", "ballot", "partial", "mix", "sballot", "smix", "pballot"):
        raise ValueError("cts belongs to kinds 'tally', 'wtally', 'ballot', 'partial', 'mix', 'sballot', 'smix' and 'pballot'")
    if weights is not None and kind != "wtally":
        raise ValueError("weights belongs to kind 'wtally'")
    for v, cnt in parts:
        if int(v) < 0 or int(v) >> (limb_bits * cnt):
            raise ValueError("a value does not fit its %d limbs" % cnt)
    out = [x for v, cnt in parts for x in limbs(v, cnt)]
    if kind == "wtally":      # the weights stand between the ciphertexts and the result
        out[-2 * Ln:-2 * Ln] = [int(v) for v in weights]
    if total is not None:
        out.append(int(total))
    if totals is not None:
        out += [int(t) for t in totals]
    return out


def instance_eval(k: int, values: Sequence[int], x: int) -> int:
    """the instance column at x: sum_i v_i l_i(x), l_i(x) = (x^n - 1)/n w^i / (x - w^i); x must not lie on the domain"""
    n = 1 << k
    w = consts.fr_omega(k)
    acc, wi = 0, 1
    for v in values:
        acc = (acc + v * wi % R * pow((x - wi) % R, -1, R)) % R
        wi = wi * w % R
    return acc * ((pow(x, n, R) - 1) % R) % R * pow(n, -1, R) % R


def replay_transcript(seed: bytes, com: Dict[str, np.ndarray], ev: Dict[str, np.ndarray], instances: Optional[Sequence[int]] = None) -> Dict[str, int]:
    h = hashlib.blake2b(bytes(seed), digest_size=64, person=b"Halo2-Transcript")
    out: Dict[str, int] = {}
    for v in instances or ():            # the statement: scalars (tag 2, Montgomery words) after the seed, before the first commitment
        h.update(b"\x02" + struct.pack("<4Q", *(int(x) for x in consts.fr_mont_limbs(int(v)))))

    def items(tag, a, words):
        a = np.ascontiguousarray(a, dtype="<u8").reshape(-1, words)
        for row in a:
            h.update(bytes([tag]) + struct.pack("<%dQ" % words, *(int(x) for x in row)))

    def draw(name):
        h.update(b"\x00")
        out[name] = int.from_bytes(h.copy().digest(), "little") % R

    for fams, names in COMMITMENT_ROUNDS:
        for f in fams:
            items(1, com[f], 8)
        for nm in names:
            draw(nm)
    for f in EVAL_FAMILIES:
        items(2, ev[f], 4)
        if f == "lookup_advice" and "constants" in ev:
            items(2, ev["constants"], 4)
    draw("sh_y")
    draw("sh_v")
    items(1, com["w1"], 8)
    draw("sh_u")
    return out


def _lagrange(k: int, bf: int, x: int) -> Tuple[int, int, int]:
    """l_0(x), l_last(x), sum of the blinding rows' l_i(x)"""
    n = 1 << k
    w = consts.fr_omega(k)
    xn1 = (pow(x, n, R) - 1) % R

    def li(i):
        wi = pow(w, i, R)
        return xn1 * wi % R * pow(n * (x - wi) % R, -1, R) % R

    u = n - (bf + 1)
    return li(0), li(u), sum(li(i) for i in range(u + 1, n)) % R


def constraint_expression(vk: VerifyingKey, e: Dict[str, List[List[int]]], beta: int, gamma: int, y: int, x: int,
                          inst_x: Optional[int] = None) -> int:
    """the constraint lines of these circuits at x folded by y (halo2's expressions in the order the prover folds them): equals
    h(x) (x^n - 1) for an honest proof.  inst_x: the instance column at x (instance_eval), the last permuted value of a key that has one"""
    A, Lk = vk.n_adv, vk.n_lk
    l0, llast, lblind = _lagrange(vk.k, vk.blinding_factors, x)
    lact = (1 - llast - lblind) % R
    acc = 0

    def line(v):
        nonlocal acc
        acc = (acc * y + v) % R

    for j in range(A):                                   # q (a + b c - d) over four rows
        a0, a1, a2, a3 = e["advice"][j]
        line(e["fixed"][j][0] * (a0 + a1 * a2 - a3))
    vals = [e["advice"][j][0] for j in range(A)] + [e["lookup_advice"][j][0] for j in range(Lk)] + [e["fixed"][A][0]]
    if inst_x is not None:
        vals.append(inst_x % R)
    m = len(vals)
    S = -(-m // CHUNK)
    z = e["perm_z"]
    line(l0 * (1 - z[0][0]))
    line(llast * (z[S - 1][0] * z[S - 1][0] - z[S - 1][0]))
    for j in range(1, S):
        line(l0 * (z[j][0] - z[j - 1][2]))
    cur = beta * x % R
    for j in range(S):
        left, right = z[j][1], z[j][0]
        for c in range(j * CHUNK, min(m, (j + 1) * CHUNK)):
            left = left * (vals[c] + beta * e["sigma"][c][0] + gamma) % R
            right = right * (vals[c] + cur + gamma) % R
            cur = cur * DELTA % R
        line(lact * (left - right))
    tab = e["fixed"][A + 1][0]
    for j in range(Lk):
        a = e["lookup_advice"][j][0]
        zx, zwx = e["lookup_z"][j]
        ap, ap_prev = e["perm_inputs"][j]
        sp = e["perm_tables"][j][0]
        line(l0 * (1 - zx))
        line(llast * (zx * zx - zx))
        line(lact * (zwx * (ap + beta) % R * (sp + gamma) - zx * (a + beta) % R * (tab + gamma)))
        line(l0 * (ap - sp))
        line(lact * (ap - sp) % R * (ap - ap_prev))
    return acc


def _interp_eval(xs: Sequence[int], ys: Sequence[int], u: int) -> int:
    """the interpolating polynomial of (xs, ys) at u (Lagrange form)"""
    acc = 0
    for i, xi in enumerate(xs):
        num, den = 1, 1
        for j, xj in enumerate(xs):
            if j != i:
                num = num * (u - xj) % R
                den = den * (xi - xj) % R
        acc = (acc + ys[i] * num * pow(den, -1, R)) % R
    return acc


@dataclass
class _Terms:
    ok: bool                      # transcript shape and the identity at x
    vk_scalars: np.ndarray        # object array of ints: fixed (F) then sigma (m), coefficients of A
    g_scalar: int                 # coefficient of g[0] in A
    bases: np.ndarray             # (count, 8) the proof's own points
    a_scalars: List[int]          # their coefficients in A
    b_scalars: List[int]          # ... in B


def _terms(vk: VerifyingKey, com: Dict[str, np.ndarray], ev: Dict[str, np.ndarray], seed: bytes, instances: Optional[Sequence[int]] = None) -> _Terms:
    A, Lk, m, S = vk.n_adv, vk.n_lk, vk.m, vk.n_sets
    F = A + 2
    shapes = {"advice": (A, 4), "lookup_advice": (Lk, 1), "fixed": (F, 1), "sigma": (m, 1), "perm_z": (S, 3), "lookup_z": (Lk, 2),
              "perm_inputs": (Lk, 2), "perm_tables": (Lk, 1), "random": (1, 1)}
    cshapes = {"advice": A, "lookup_advice": Lk, "perm_inputs": Lk, "perm_tables": Lk, "perm_z": S, "lookup_z": Lk, "random": 1,
               "h": H_PIECES, "w1": 1, "w2": 1}
    bad = _Terms(False, np.zeros(F + m, dtype=object), 0, np.zeros((0, 8), dtype=np.uint64), [], [])
    try:
        for f, (cnt, pts) in shapes.items():
            if tuple(np.asarray(ev[f]).shape) != (cnt, pts, 4):
                return bad
        for f, cnt in cshapes.items():
            if tuple(np.asarray(com[f]).shape) != (cnt, 8):
                return bad
    except KeyError:
        return bad
    # words nobody has decoded: a commitment off the curve or with a coordinate that is not canonical, or an evaluation >= r, refuses
    # the proof (the device verifier's rule, pz_verify_batch; never laxer than the wire decoder)
    if not all(_points_ok(com[f]) for f in cshapes) or not all(_evals_canonical(ev[f]) for f in ev if f in shapes or f in ("constants", "h")):
        return bad
    inst = [int(v) for v in instances] if vk.n_instance else None
    if inst is not None and any(not 0 <= v < R for v in inst):
        return bad                                         # a value >= r is no statement
    ch = replay_transcript(seed, com, ev, inst)
    e = {f: _ints(ev[f]) for f in shapes}
    x = ch["x"]
    n = 1 << vk.k
    xn = pow(x, n, R)
    if xn == 1:
        return bad                                         # a challenge on the domain
    inst_x = instance_eval(vk.k, inst, x) if inst is not None else None
    h_eval = constraint_expression(vk, e, ch["beta"], ch["gamma"], ch["y"], x, inst_x) * pow(xn - 1, -1, R) % R
    ok = True
    if "h" in ev:                                          # a proof that states h(x) must state the expected one
        ok = _ints(ev["h"]) == [[h_eval]]
    e["h"] = [[h_eval]]
    dom = Domain(vk.k, vk.blinding_factors)
    points = rotation_points(dom, x)
    sy, sv, su = ch["sh_y"], ch["sh_v"], ch["sh_u"]
    zt = 1
    for t in points:
        zt = zt * (su - t) % R
    vk_sc = np.zeros(F + m, dtype=object)
    vk_sc[:] = 0
    g_sc = 0
    bases, a_sc, b_sc = [], [], []
    z0 = None
    for kk, (idx, members) in enumerate(query_layout(A, Lk, m, S)):
        zk = 1
        for t, pt in enumerate(points):
            if t not in idx:
                zk = zk * (su - pt) % R
        if kk == 0:
            z0 = zk
        xs = [points[i] for i in idx]
        folded = [sum(pow(sy, j, R) * e[f][i][q] for j, (f, i) in enumerate(members)) % R for q in range(len(xs))]
        coef = pow(sv, kk, R) * zk % R
        g_sc = (g_sc - coef * _interp_eval(xs, folded, su)) % R
        for j, (f, i) in enumerate(members):
            c = coef * pow(sy, j, R) % R
            if f == "fixed":
                vk_sc[i] = (vk_sc[i] + c) % R
            elif f == "sigma":
                vk_sc[F + i] = (vk_sc[F + i] + c) % R
            elif f == "h":                                 # [h] = sum_i x^(n i) [h_i]
                for p in range(H_PIECES):
                    bases.append(com["h"][p])
                    a_sc.append(c * pow(xn, p, R) % R)
                    b_sc.append(0)
            else:
                bases.append(com[f][i])
                a_sc.append(c)
                b_sc.append(0)
    bases.append(com["w1"][0])
    a_sc.append((-zt) % R)
    b_sc.append(0)
    bases.append(com["w2"][0])
    a_sc.append(z0 * su % R)
    b_sc.append((-z0) % R)
    return _Terms(ok, vk_sc, g_sc, np.stack([np.asarray(b, dtype=np.uint64).reshape(8) for b in bases]), a_sc, b_sc)


def _mont(vals: Sequence[int]) -> np.ndarray:
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        out[i] = consts.fr_mont_limbs(int(v))
    return out


def _fold_and_check(eng, params: VerifierParams, vk: VerifyingKey, terms: Sequence[_Terms], cols: Sequence[Sequence[int]]) -> List[int]:
    """cols: per column of the MSM the weight of each proof (len(terms)) and whether it is the A or the B side -> pairing checks of
    (A_c, B_c) pairs: column 2c is A, 2c + 1 is B; returns d_ok"""
    F_m = len(terms[0].vk_scalars)
    bases = np.concatenate([vk.fixed.reshape(-1, 8), vk.sigma.reshape(-1, 8), params.g0.reshape(1, 8)] + [t.bases for t in terms])
    nb = bases.shape[0]
    n_cols = len(cols)
    sc = [[0] * nb for _ in range(n_cols)]
    for c, (side, weights) in enumerate(cols):
        row = sc[c]
        off = F_m + 1
        for t, wgt in zip(terms, weights):
            if wgt:
                if side == 0:
                    for i in range(F_m):
                        row[i] = (row[i] + wgt * t.vk_scalars[i]) % R
                    row[F_m] = (row[F_m] + wgt * t.g_scalar) % R
                src = t.a_scalars if side == 0 else t.b_scalars
                for i, s in enumerate(src):
                    row[off + i] = wgt * s % R
            off += t.bases.shape[0]
    scal = np.concatenate([_mont(r) for r in sc])
    nbytes_b, nbytes_s = nb * 64, scal.nbytes
    d = eng.dev_alloc(nbytes_b + nbytes_s + n_cols * 96 + n_cols * 64 + (n_cols // 2) * 2 * 128 + 4 * n_cols)
    try:
        d_b, d_s = d, d + nbytes_b
        d_jac = d_s + nbytes_s
        d_g1 = d_jac + n_cols * 96
        d_g2 = d_g1 + n_cols * 64
        d_ok = d_g2 + (n_cols // 2) * 2 * 128
        eng.upload(d_b, bases)
        eng.upload(d_s, scal)
        tb = eng.load_bases_dev(d_b, nb)
        try:
            eng.msm_dev(tb, d_s, n_cols, nb, 4 * nb, d_jac)
            aff = eng.g1_normalize(eng.download(d_jac, (n_cols, 12)))
        finally:
            tb.free()
        n_checks = n_cols // 2
        g2s = np.tile(np.concatenate([params.g2, params.s_g2]).reshape(1, 2, 16), (n_checks, 1, 1))
        eng.upload(d_g1, np.ascontiguousarray(aff))
        eng.upload(d_g2, g2s)
        eng.pairing_check_dev(d_g1, d_g2, n_checks, 2, d_ok)
        return [int(v) for v in eng.download(d_ok, n_checks, np.int32)]
    finally:
        eng.dev_free(d)


def _as_parts(proof, vk: VerifyingKey):
    if isinstance(proof, tuple):                      # (read_proofs record, "p<i>/")
        return proof_from_record(proof[0], proof[1], vk)
    return proof.commitments, proof.evals


def _check_instances(vk: VerifyingKey, instances, B: int):
    """-> one list of public values per proof (None for a key without the instance column); ValueError on a wrong count"""
    if not vk.n_instance:
        if instances is not None:
            raise ValueError("this key has no instance column")
        return [None] * B
    if instances is None or len(instances) != B or any(len(v) != vk.n_public for v in instances):
        raise ValueError("this key's statement has %d public values per proof" % vk.n_public)
    return [list(v) for v in instances]


def verify_batch(eng, params: VerifierParams, vk: VerifyingKey, proofs: Sequence, seeds: Sequence[bytes], instances=None,
                 bind_key: bool = False) -> Tuple[bool, List[bool]]:
    """-> (every proof holds, per-proof verdicts).  proofs: prover.Proof objects or (prover_job.read_proofs record, "p<i>/") pairs; seeds:
    the transcript seed of each (record_seed for the compiled prover's).  params: VerifierParams (or a srs.ParamsKZG, whose G2 elements must not be zero).
    instances: per proof the list of its public values (public_inputs) when the key has an instance column.
    bind_key: replay every transcript from vk.digest() + seed (proofs made with HashTranscript(seed, key_digest=...))."""
    if not isinstance(params, VerifierParams):
        params = VerifierParams.from_params(params)
    assert len(proofs) == len(seeds) and len(proofs) > 0
    inst = _check_instances(vk, instances, len(proofs))
    if bind_key:
        D = vk.digest()
        seeds = [D + bytes(sd) for sd in seeds]
    terms = [_terms(vk, *_as_parts(p, vk), s, iv) for p, s, iv in zip(proofs, seeds, inst)]
    B = len(terms)
    idents = [t.ok for t in terms]
    live = [i for i in range(B) if terms[i].bases.shape[0]]
    if not live:
        return False, [False] * B
    lt = [terms[i] for i in live]
    if all(idents):
        r = [int.from_bytes(os.urandom(32), "little") % R for _ in lt]
        (ok,) = _fold_and_check(eng, params, vk, lt, [(0, r), (1, r)])
        if ok == 1:
            return True, [True] * B
    # per proof: B independent checks in one launch
    cols = []
    for j in range(len(lt)):
        w = [1 if q == j else 0 for q in range(len(lt))]
        cols += [(0, w), (1, w)]
    res = _fold_and_check(eng, params, vk, lt, cols)
    per = [False] * B
    for j, i in enumerate(live):
        per[i] = idents[i] and res[j] == 1
    return all(per), per


def verify_proof(eng, params, vk: VerifyingKey, proof, seed: bytes, instances=None, bind_key: bool = False) -> bool:
    return verify_batch(eng, params, vk, [proof], [seed], None if instances is None else [instances], bind_key=bind_key)[0]


# ---- the device batch verifier (include/pz.h: pz_vk_create / pz_verify_batch): the same verdicts, Fr work in HIP ----------------------
PROOF_COMMITMENTS = ("advice", "lookup_advice", "perm_inputs", "perm_tables", "perm_z", "lookup_z", "random", "h", "w1", "w2")
PROOF_EVALS = ("advice", "lookup_advice", "constants", "fixed", "sigma", "perm_z", "lookup_z", "perm_inputs", "perm_tables", "random", "h")


def native_key(eng, params, vk: VerifyingKey):
    """-> engine.VkHandle of the key and the params' g[0], g2, s_g2 (pz_vk_create refuses zero G2 and an identity g[0])"""
    if not isinstance(params, VerifierParams):
        params = VerifierParams.from_params(params)
    return eng.vk_create(vk.k, vk.blinding_factors, vk.n_adv, vk.n_lk, vk.fixed, vk.sigma, params.g0, params.g2, params.s_g2, vk.n_instance,
                         vk.n_public)


def pack_proof(vk: VerifyingKey, com: Dict[str, np.ndarray], ev: Dict[str, np.ndarray]):
    """a proof's commitments and evaluations -> its words in pz_verify_batch's layout (the stepper's outputs in phase order), or None if a
    family is missing or has the wrong shape"""
    A, Lk, m, S = vk.n_adv, vk.n_lk, vk.m, vk.n_sets
    cshapes = (A, Lk, Lk, Lk, S, Lk, 1, H_PIECES, 1, 1)
    eshapes = ((A, 4), (Lk, 1), (1, 1), (A + 2, 1), (m, 1), (S, 3), (Lk, 2), (Lk, 2), (Lk, 1), (1, 1), (1, 1))
    try:
        parts = []
        for f, cnt in zip(PROOF_COMMITMENTS, cshapes):
            a = np.asarray(com[f], dtype=np.uint64)
            if a.shape != (cnt, 8):
                return None
            parts.append(a.reshape(-1))
        for f, (cnt, pts) in zip(PROOF_EVALS, eshapes):
            a = np.asarray(ev[f], dtype=np.uint64)
            if a.shape != (cnt, pts, 4):
                return None
            parts.append(a.reshape(-1))
    except KeyError:
        return None
    return np.concatenate(parts)


def _bound(handle, bind_key: bool, fn):
    """fn() with the handle's binding (pz_vk_bind) set to bind_key; a caller's handle gets its own setting back"""
    was = handle.bound
    if was != bool(bind_key):
        handle.bind(bind_key)
    try:
        return fn()
    finally:
        if was != bool(bind_key):
            handle.bind(was)


def verify_batch_native(eng, params, vk: VerifyingKey, proofs: Sequence, seeds: Sequence[bytes], handle=None, instances=None,
                        bind_key: bool = False) -> Tuple[bool, List[bool]]:
    """verify_batch on the device batch verifier: the same arguments and (every proof holds, per-proof verdicts).  handle: a native_key
    of (params, vk) to reuse; made and freed here otherwise.  bind_key: pz_vk_bind for this call (the library hashes its own digest of the
    key in front of every seed)."""
    assert len(proofs) == len(seeds) and len(proofs) > 0
    inst = _check_instances(vk, instances, len(proofs))
    packed = [pack_proof(vk, *_as_parts(p, vk)) for p in proofs]
    live = [i for i, w in enumerate(packed) if w is not None]
    per = [False] * len(proofs)
    if not live:
        return False, per
    own = handle is None
    h = native_key(eng, params, vk) if own else handle
    try:
        _, got, _, _ = _bound(h, bind_key, lambda: eng.verify_batch_dev(h, np.stack([packed[i] for i in live]), [seeds[i] for i in live],
                                                                        instances=[inst[i] for i in live] if vk.n_instance else None))
    finally:
        if own:
            h.free()
    for i, v in zip(live, got):
        per[i] = v
    return all(per), per


# ---- halo2 wire bytes (include/pz.h: pz_g1_*compress, pz_proof_encode / decode, pz_verify_batch_bytes) ----------
VK_MAGIC = b"PZVK"
VK_VERSION = 1
VK_VERSION_PUB = 2        # a key with the instance column: two more header words, n_instance and n_public


def _proof_shapes(vk: VerifyingKey):
    A, Lk, m, S = vk.n_adv, vk.n_lk, vk.m, vk.n_sets
    cshapes = (A, Lk, Lk, Lk, S, Lk, 1, H_PIECES, 1, 1)
    eshapes = ((A, 4), (Lk, 1), (1, 1), (A + 2, 1), (m, 1), (S, 3), (Lk, 2), (Lk, 2), (Lk, 1), (1, 1), (1, 1))
    return cshapes, eshapes


def proof_size_bytes(vk: VerifyingKey) -> int:
    """a proof as halo2 wire bytes: 32 per commitment and per evaluation; h(x) is not sent"""
    cshapes, eshapes = _proof_shapes(vk)
    return 32 * (sum(cshapes) + sum(c * p for c, p in eshapes) - 1)


def _codec_key(eng, vk: VerifyingKey):
    """a VkHandle for the proof codec alone: the wire layout depends on the key's shape only, so the generators stand in for the params"""
    g1 = np.concatenate([consts.int_to_limbs(v * consts.MONT_R % consts.FQ_P, 4) for v in (1, 2)]).astype(np.uint64)
    g2 = eng.g2_generator()
    return eng.vk_create(vk.k, vk.blinding_factors, vk.n_adv, vk.n_lk, vk.fixed, vk.sigma, g1, g2, g2, vk.n_instance, vk.n_public)


def _with_key(eng, vk, handle, fn):
    own = handle is None
    h = _codec_key(eng, vk) if own else handle
    try:
        return fn(h)
    finally:
        if own:
            h.free()


def proof_to_bytes(eng, vk: VerifyingKey, proof, handle=None) -> bytes:
    """a proof (prover.Proof or a (record, prefix) pair) -> its halo2 wire bytes, encoded on the device"""
    com, ev = _as_parts(proof, vk)
    ev = dict(ev)
    ev.setdefault("h", np.zeros((1, 1, 4), dtype=np.uint64))      # not sent
    words = pack_proof(vk, com, ev)
    if words is None:
        raise ValueError("the proof does not have the key's shape")
    return _with_key(eng, vk, handle, lambda h: eng.proof_encode(h, words)[0].tobytes())


def _unpack_words(vk: VerifyingKey, words: np.ndarray):
    from .prover import Proof

    cshapes, eshapes = _proof_shapes(vk)
    com, ev, o = {}, {}, 0
    for f, cnt in zip(PROOF_COMMITMENTS, cshapes):
        com[f] = words[o:o + 8 * cnt].reshape(cnt, 8).copy()
        o += 8 * cnt
    for f, (cnt, pts) in zip(PROOF_EVALS, eshapes):
        if f != "h":
            ev[f] = words[o:o + 4 * cnt * pts].reshape(cnt, pts, 4).copy()
        o += 4 * cnt * pts
    return Proof(commitments=com, evals=ev)


def proof_from_bytes(eng, vk: VerifyingKey, data: bytes, handle=None):
    """halo2 wire bytes -> prover.Proof (its evals carry "constants" as a family of its own and no "h": the verifier computes h(x)).
    ValueError if the length is wrong or an element does not decode."""
    if len(data) != proof_size_bytes(vk):
        raise ValueError("a proof of this key is %d bytes, got %d" % (proof_size_bytes(vk), len(data)))
    words, st = _with_key(eng, vk, handle, lambda h: eng.proof_decode(h, np.frombuffer(bytes(data), dtype=np.uint8)))
    if int(st[0]) != 0:
        raise ValueError("the proof does not decode: %s" % ("an element is not canonical" if st[0] == 1 else "a point is not on the curve"))
    return _unpack_words(vk, words[0])


def vk_to_bytes(eng, vk: VerifyingKey) -> bytes:
    """"PZVK", u32 version, k, blinding_factors, n_adv, n_lk, then the fixed and the sigma commitments compressed.  A key with the instance
    column is version 2: n_instance and n_public follow n_lk (a key without it gives version 1, byte for byte what it always gave)"""
    pts = np.concatenate([np.asarray(vk.fixed, dtype=np.uint64).reshape(-1, 8), np.asarray(vk.sigma, dtype=np.uint64).reshape(-1, 8)])
    if pts.shape[0] != 2 * vk.n_adv + vk.n_lk + 3 + vk.n_instance:
        raise ValueError("fixed must hold n_adv + 2 points and sigma n_adv + n_lk + 1 (+ 1 with an instance column)")
    if vk.n_instance:
        return VK_MAGIC + struct.pack("<7I", VK_VERSION_PUB, vk.k, vk.blinding_factors, vk.n_adv, vk.n_lk, vk.n_instance, vk.n_public) + \
            eng.g1_compress(pts).tobytes()
    return VK_MAGIC + struct.pack("<5I", VK_VERSION, vk.k, vk.blinding_factors, vk.n_adv, vk.n_lk) + eng.g1_compress(pts).tobytes()


def vk_from_bytes(eng, data: bytes) -> VerifyingKey:
    data = bytes(data)
    if len(data) < 24 or data[:4] != VK_MAGIC:
        raise ValueError("not a verifying key file")
    ver, k, bf, A, Lk = struct.unpack("<5I", data[4:24])
    hdr, ni, npub = 24, 0, 0
    if ver == VK_VERSION_PUB:
        if len(data) < 32:
            raise ValueError("not a verifying key file")
        ni, npub = struct.unpack("<2I", data[24:32])
        hdr = 32
        if ni != 1 or npub == 0:
            raise ValueError("a version-2 key has one instance column and at least one public value")
    elif ver != VK_VERSION:
        raise ValueError("verifying key file version %d" % ver)
    n = 2 * A + Lk + 3 + ni
    if len(data) != hdr + 32 * n:
        raise ValueError("a key of this shape is %d bytes, got %d" % (hdr + 32 * n, len(data)))
    pts, st = eng.g1_decompress(data[hdr:])
    if st.any():
        raise ValueError("%d of the key's points do not decode" % int(np.count_nonzero(st)))
    return VerifyingKey(k, bf, A, Lk, -(-(A + Lk + 1 + ni) // CHUNK), pts[:A + 2].copy(), pts[A + 2:].copy(), ni, npub)


def verify_batch_bytes(eng, params, vk: VerifyingKey, proofs: Sequence[bytes], seeds: Sequence[bytes], handle=None, instances=None,
                       bind_key: bool = False) -> Tuple[bool, List[bool]]:
    """verify_batch for proofs that arrive as halo2 wire bytes (pz_verify_batch_bytes: decoded on the device; a proof that does not decode
    is False and the others are judged without it).  ValueError if a proof's length is not proof_size_bytes(vk).  bind_key: pz_vk_bind for
    this call."""
    assert len(proofs) == len(seeds) and len(proofs) > 0
    inst = _check_instances(vk, instances, len(proofs))
    size = proof_size_bytes(vk)
    for p in proofs:
        if len(p) != size:
            raise ValueError("a proof of this key is %d bytes, got %d" % (size, len(p)))
    data = np.frombuffer(b"".join(bytes(p) for p in proofs), dtype=np.uint8)
    own = handle is None
    h = native_key(eng, params, vk) if own else handle
    try:
        ok, per, _, _ = _bound(h, bind_key, lambda: eng.verify_batch_bytes_dev(h, data, seeds, instances=inst if vk.n_instance else None))
    finally:
        if own:
            h.free()
    return ok, per
