"""Thin host-side handle over the C ABI (include/pz.h): owns a pz_ctx, marshals numpy arrays
(host-pointer entry points) and torch CUDA tensors (device-pointer entry points).

All arithmetic happens in libpz_hip.so on the MI355X.  Array conventions are the ABI's: uint64,
field elements (…,4) Montgomery limbs, affine points (…,8), Jacobian points (…,12), big
integers little-endian u64 limbs.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import PzError, VP

# pz_msm_g1_dev_ex's density hint (include/pz.h PZ_MSM_*)
MSM_AUTO, MSM_SPARSE, MSM_DENSE = 0, 1, 2


def _np(a, shape_last: Optional[int] = None) -> np.ndarray:
    arr = np.ascontiguousarray(a, dtype=np.uint64)
    if shape_last is not None and (arr.ndim == 0 or arr.shape[-1] != shape_last):
        arr = arr.reshape(-1, shape_last)
    return arr


def _ptr(a: np.ndarray) -> VP:
    return VP(a.ctypes.data)


class Bases:
    """A device-resident window-shifted base table (pz_bases)."""

    def __init__(self, engine: "Engine", handle: VP):
        self.engine = engine
        self.handle = handle
        n = C.c_size_t()
        c = C.c_uint32()
        w = C.c_uint32()
        engine._chk(_lib.lib().pz_bases_info(handle, C.byref(n), C.byref(c), C.byref(w)), "pz_bases_info")
        self.n_points = n.value
        self.window_bits = c.value
        self.n_windows = w.value

    def free(self):
        if self.handle is not None:
            _lib.lib().pz_bases_free(self.engine.ctx, self.handle)
            self.handle = None


class VkHandle:
    """A verifying key on the device (pz_vk): the key's commitments, g[0] and the G2 pair; frees itself."""

    def __init__(self, engine: "Engine", handle: VP):
        self.engine = engine
        self.handle = handle
        cw, ew = C.c_size_t(), C.c_size_t()
        engine._chk(_lib.lib().pz_vk_info(handle, C.byref(cw), C.byref(ew)), "pz_vk_info")
        self.commitment_words, self.evals_words = cw.value, ew.value

    @property
    def proof_words(self) -> int:
        return self.commitment_words + self.evals_words

    @property
    def wire_bytes(self) -> int:
        """a proof's size as halo2 wire bytes (pz_proof_wire_bytes)"""
        n = C.c_size_t()
        self.engine._chk(_lib.lib().pz_proof_wire_bytes(self.handle, C.byref(n)), "pz_proof_wire_bytes")
        return n.value

    def digest(self) -> bytes:
        """pz_vk_digest: the key's 64-byte digest (prover.key_digest's function; computed once per handle)"""
        out = (C.c_uint8 * 64)()
        self.engine._chk(_lib.lib().pz_vk_digest(self.handle, out), "pz_vk_digest")
        return bytes(out)

    def bind(self, on: bool = True):
        """pz_vk_bind: every verification through this handle replays each proof from digest || seed (off: from the seed alone)"""
        self.engine._chk(_lib.lib().pz_vk_bind(self.handle, 1 if on else 0), "pz_vk_bind")

    @property
    def bound(self) -> bool:
        on = C.c_int()
        self.engine._chk(_lib.lib().pz_vk_is_bound(self.handle, C.byref(on)), "pz_vk_is_bound")
        return bool(on.value)

    def free(self):
        if self.handle is not None:
            _lib.lib().pz_vk_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _BorrowedBases(Bases):
    """a base table owned by a params object: valid while that object lives, not freed here"""

    def __init__(self, engine: "Engine", handle: VP, owner):
        super().__init__(engine, handle)
        self.owner = owner

    def free(self):
        self.handle = None


class ParamsHandle:
    """A ParamsKZG on the device (pz_params): g, g_lagrange, the G2 pair and, on request, their window tables; frees itself."""

    def __init__(self, engine: "Engine", handle: VP):
        self.engine = engine
        self.handle = handle
        self._bases = {}
        k = C.c_uint32()
        engine._chk(_lib.lib().pz_params_info(handle, C.byref(k), None, None, None), "pz_params_info")
        self.k = k.value

    def info(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(g[0] (8 words), g2 (16), s_g2 (16)): what pz_vk_create takes"""
        g0, g2, s_g2 = np.zeros(8, dtype=np.uint64), np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
        self.engine._chk(_lib.lib().pz_params_info(self.handle, None, _ptr(g0), _ptr(g2), _ptr(s_g2)), "pz_params_info")
        return g0, g2, s_g2

    def points(self) -> Tuple[int, int]:
        """device pointers of g and g_lagrange (2^k affine points each), owned by the object"""
        a, b = VP(), VP()
        self.engine._chk(_lib.lib().pz_params_points(self.handle, C.byref(a), C.byref(b)), "pz_params_points")
        return a.value or 0, b.value or 0

    def bases(self, lagrange: bool) -> Bases:
        key = bool(lagrange)
        if key not in self._bases:
            h = VP()
            self.engine._chk(_lib.lib().pz_params_bases(self.handle, int(key), C.byref(h)), "pz_params_bases")
            self._bases[key] = _BorrowedBases(self.engine, h, self)
        return self._bases[key]

    def encode(self, fmt: int) -> np.ndarray:
        out = np.zeros(self.engine.params_file_bytes(self.k, fmt), dtype=np.uint8)
        self.engine._chk(_lib.lib().pz_params_encode(self.handle, fmt, VP(out.ctypes.data), out.size), "pz_params_encode")
        return out

    def downsize(self, k_new: int) -> "ParamsHandle":
        h = VP()
        self.engine._chk(_lib.lib().pz_params_downsize(self.handle, k_new, C.byref(h)), "pz_params_downsize")
        return ParamsHandle(self.engine, h)

    def check(self) -> Tuple[int, int]:
        """(failed, skipped): pz_params_check's bit sets (PZ_PARAMS_BAD_*)"""
        f, s = C.c_uint32(), C.c_uint32()
        self.engine._chk(_lib.lib().pz_params_check(self.handle, C.byref(f), C.byref(s)), "pz_params_check")
        return f.value, s.value

    def free(self):
        if self.handle is not None:
            for b in self._bases.values():
                b.free()
            _lib.lib().pz_params_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    """One pz_ctx == one GPU (one process per GPU; ranks are joined by RCCL above this layer)."""

    def __init__(self, device: int = 0):
        self.L = _lib.lib()
        self.ctx = VP()
        dev = (C.c_int * 1)(device)
        rc = self.L.pz_init(1, dev, C.byref(self.ctx))
        if rc != 0:
            raise PzError(rc, "pz_init")
        self.device = device

    # ------------------------------------------------------------------ plumbing
    def _chk(self, rc: int, where: str):
        if rc != 0:
            detail = self.L.pz_last_hip_error(self.ctx).decode() if self.ctx else ""
            raise PzError(rc, where, detail)

    def last_hip_error(self) -> str:
        """pz_last_hip_error: the text of the context's last failed HIP call or device-side complaint, "" if there was none"""
        return self.L.pz_last_hip_error(self.ctx).decode() if self.ctx else ""

    def close(self):
        if self.ctx:
            self.L.pz_free(self.ctx)
            self.ctx = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle: int = 0):
        """stream_handle: a raw hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); 0 = own."""
        self._chk(self.L.pz_set_stream(self.ctx, VP(stream_handle)), "pz_set_stream")

    def bind_torch_stream(self, stream=None):
        """Run the library on a torch stream (a fresh one by default) and make that stream torch's current one, so
        torch fills / copies / event waits and the library's kernels are ordered.  torch's DEFAULT stream is the NULL
        stream, whose handle 0 means "the library's own non-blocking stream" to pz_set_stream -- binding to it
        orders nothing."""
        import torch

        if stream is None:
            stream = torch.cuda.Stream(device=self.device)
        assert stream.cuda_stream != 0
        torch.cuda.set_stream(stream)
        self.set_stream(stream.cuda_stream)
        self._torch_stream = stream
        return stream

    def sync(self):
        self._chk(self.L.pz_sync(self.ctx), "pz_sync")

    # ------------------------------------------------------------------ K1: MSM
    def load_bases(self, bases_affine, window_bits: int = 0) -> Bases:
        b = _np(bases_affine, 8)
        h = VP()
        self._chk(self.L.pz_bases_load_g1(self.ctx, _ptr(b), b.shape[0], 0, window_bits, C.byref(h)),
                  "pz_bases_load_g1")
        return Bases(self, h)

    def load_bases_dev(self, d_ptr: int, n_points: int, window_bits: int = 0) -> Bases:
        h = VP()
        self._chk(self.L.pz_bases_load_g1(self.ctx, VP(d_ptr), n_points, 1, window_bits, C.byref(h)),
                  "pz_bases_load_g1(dev)")
        return Bases(self, h)

    def srs_load_g1(self, k: int, bases_affine, lagrange: bool = False) -> Bases:
        b = _np(bases_affine, 8)
        assert b.shape[0] == 1 << k
        h = VP()
        self._chk(self.L.pz_srs_load_g1(self.ctx, k, _ptr(b), int(lagrange), C.byref(h)), "pz_srs_load_g1")
        return Bases(self, h)

    def msm(self, bases: Bases, scalars) -> np.ndarray:
        s = _np(scalars, 4)
        out = np.zeros(12, dtype=np.uint64)
        self._chk(self.L.pz_msm_g1(self.ctx, bases.handle, _ptr(s) if s.size else VP(), s.shape[0] if s.size else 0,
                                   _ptr(out)), "pz_msm_g1")
        return out

    def msm_batch(self, bases: Bases, cols: Sequence[np.ndarray]) -> np.ndarray:
        cols = [_np(c, 4) for c in cols]
        n = cols[0].shape[0] if cols else 0
        assert all(c.shape[0] == n for c in cols)
        arr = (VP * len(cols))(*[_ptr(c) for c in cols])
        out = np.zeros((len(cols), 12), dtype=np.uint64)
        self._chk(self.L.pz_msm_g1_batch(self.ctx, bases.handle, arr, len(cols), n, _ptr(out)), "pz_msm_g1_batch")
        return out

    def msm_dev(self, bases: Bases, d_scalars: int, n_cols: int, n: int, col_stride_u64: int, d_out: int,
                win_lo: int = 0, win_hi: Optional[int] = None, density: Optional[int] = None):
        """density: None (MSM_AUTO: the device picks the sort variant per launch), MSM_SPARSE (columns of short scalars) or
        MSM_DENSE (full-width scalars) -- pz_msm_g1_dev_ex's hint: it chooses launches, never results"""
        if win_hi is None:
            win_hi = bases.n_windows
        self._chk(self.L.pz_msm_g1_dev_ex(self.ctx, bases.handle, VP(d_scalars), n_cols, n, col_stride_u64, win_lo,
                                          win_hi, MSM_AUTO if density is None else int(density), VP(d_out)), "pz_msm_g1_dev_ex")

    @staticmethod
    def msm_multi(engines: Sequence["Engine"], bases: Sequence[Bases], d_scalars: Sequence[int], n_per_ctx: Sequence[int],
                  split_points: bool) -> np.ndarray:
        """pz_msm_g1_multi: ONE MSM over several contexts (one per GPU; several on one device for rehearsal).  d_scalars: device
        pointers, one per context.  Returns the Jacobian point (12,)."""
        k = len(engines)
        assert len(bases) == len(d_scalars) == len(n_per_ctx) == k and k > 0
        ctxs = (VP * k)(*[e.ctx for e in engines])
        bs = (VP * k)(*[(b.handle if b is not None else VP()) for b in bases])
        sc = (VP * k)(*[VP(p) for p in d_scalars])
        ns = (C.c_size_t * k)(*n_per_ctx)
        out = np.zeros(12, dtype=np.uint64)
        engines[0]._chk(engines[0].L.pz_msm_g1_multi(ctxs, bs, sc, ns, k, int(split_points), _ptr(out)), "pz_msm_g1_multi")
        return out

    def g1_sum(self, jac) -> np.ndarray:
        j = _np(jac, 12)
        out = np.zeros(12, dtype=np.uint64)
        self._chk(self.L.pz_g1_sum(self.ctx, _ptr(j), j.shape[0], _ptr(out)), "pz_g1_sum")
        return out

    def g1_sum_dev(self, d_jac: int, n: int, d_out: int):
        self._chk(self.L.pz_g1_sum_dev(self.ctx, VP(d_jac), n, VP(d_out)), "pz_g1_sum_dev")

    def g1_normalize(self, jac) -> np.ndarray:
        j = _np(jac, 12)
        out = np.zeros((j.shape[0], 8), dtype=np.uint64)
        self._chk(self.L.pz_g1_normalize(self.ctx, _ptr(j), j.shape[0], _ptr(out)), "pz_g1_normalize")
        return out

    def g1_fixed_base_mul(self, scalars) -> np.ndarray:
        s = _np(scalars, 4)
        out = np.zeros((s.shape[0], 8), dtype=np.uint64)
        self._chk(self.L.pz_g1_fixed_base_mul(self.ctx, _ptr(s), s.shape[0], _ptr(out)), "pz_g1_fixed_base_mul")
        return out

    def g1_fixed_base_mul_dev(self, d_scalars: int, n: int, d_out: int):
        self._chk(self.L.pz_g1_fixed_base_mul_dev(self.ctx, VP(d_scalars), n, VP(d_out)), "pz_g1_fixed_base_mul_dev")

    # ------------------------------------------------------------------ K2: NTT
    def ntt(self, a, omega, log_n: int) -> np.ndarray:
        x = _np(a, 4).copy()
        assert x.shape[0] == 1 << log_n
        w = _np(omega).reshape(4)
        self._chk(self.L.pz_ntt_fr(self.ctx, _ptr(x), _ptr(w), log_n), "pz_ntt_fr")
        return x

    def ntt_batch(self, cols: Sequence[np.ndarray], omega, log_n: int):
        cols = [_np(c, 4).copy() for c in cols]
        arr = (VP * len(cols))(*[_ptr(c) for c in cols])
        w = _np(omega).reshape(4)
        self._chk(self.L.pz_ntt_fr_batch(self.ctx, arr, len(cols), _ptr(w), log_n), "pz_ntt_fr_batch")
        return cols

    def ntt_batch_inplace(self, cols: Sequence[np.ndarray], omega, log_n: int):
        """host-pointer pz_ntt_fr_batch IN PLACE on the caller's arrays (uint64, contiguous): no staging copies on the host"""
        arr = (VP * len(cols))(*[_ptr(c) for c in cols])
        w = _np(omega).reshape(4)
        self._chk(self.L.pz_ntt_fr_batch(self.ctx, arr, len(cols), _ptr(w), log_n), "pz_ntt_fr_batch")

    def ntt_to_dev(self, d_in: int, in_stride_u64: int, d_out: int, out_stride_u64: int, n_cols: int, omega, log_n: int,
                   pre_coset_g=None, post_scale=None):
        """out of place: reads d_in, writes d_out (pz_ntt_fr_to_dev)"""
        w = _np(omega).reshape(4)
        g = _np(pre_coset_g).reshape(4) if pre_coset_g is not None else None
        s = _np(post_scale).reshape(4) if post_scale is not None else None
        self._chk(self.L.pz_ntt_fr_to_dev(self.ctx, VP(d_in), in_stride_u64, VP(d_out), out_stride_u64, n_cols, _ptr(w), log_n,
                                          _ptr(g) if g is not None else VP(), _ptr(s) if s is not None else VP()),
                  "pz_ntt_fr_to_dev")

    def ntt_dev(self, d_a: int, n_cols: int, col_stride_u64: int, omega, log_n: int, pre_coset_g=None,
                post_scale=None):
        w = _np(omega).reshape(4)
        g = _np(pre_coset_g).reshape(4) if pre_coset_g is not None else None
        s = _np(post_scale).reshape(4) if post_scale is not None else None
        self._chk(self.L.pz_ntt_fr_dev(self.ctx, VP(d_a), n_cols, col_stride_u64, _ptr(w), log_n,
                                       _ptr(g) if g is not None else VP(), _ptr(s) if s is not None else VP()),
                  "pz_ntt_fr_dev")

    def ntt_extend_dev(self, d_coeff: int, n_cols: int, in_stride_u64: int, d_ext: int, out_stride_u64: int, log_n: int,
                       log_e: int, omega_n, coset_gens, scale=None):
        w = _np(omega_n).reshape(4)
        g = _np(coset_gens).reshape(-1)
        assert g.size == 4 << log_e
        sc = _np(scale).reshape(4) if scale is not None else None
        self._chk(self.L.pz_ntt_fr_extend_dev(self.ctx, VP(d_coeff), n_cols, in_stride_u64, VP(d_ext), out_stride_u64,
                                              log_n, log_e, _ptr(w), _ptr(g), _ptr(sc) if sc is not None else VP()),
                  "pz_ntt_fr_extend_dev")

    def ntt_coeff_extend_dev(self, d_values: int, n_cols: int, col_stride_u64: int, d_ext: int, out_stride_u64: int, log_n: int,
                             log_e: int, omega_n, omega_n_inv, n_inv, coset_gens):
        g = _np(coset_gens).reshape(-1)
        assert g.size == 4 << log_e
        self._chk(self.L.pz_ntt_fr_coeff_extend_dev(self.ctx, VP(d_values), n_cols, col_stride_u64, VP(d_ext), out_stride_u64, log_n,
                                                    log_e, self._fr1(omega_n), self._fr1(omega_n_inv), self._fr1(n_inv), _ptr(g)),
                  "pz_ntt_fr_coeff_extend_dev")

    def fr_convert_dev(self, d_a: int, n: int, to_mont: bool = True):
        self._chk(self.L.pz_fr_convert_dev(self.ctx, VP(d_a), n, int(to_mont)), "pz_fr_convert_dev")

    def fr_from_mask_dev(self, d_mask: int, n: int, d_out: int):
        """d_out[i] = d_mask[i] != 0 ? 1 : 0 (Montgomery), n elements (device pointers)"""
        self._chk(self.L.pz_fr_from_mask_dev(self.ctx, VP(d_mask), n, VP(d_out)), "pz_fr_from_mask_dev")

    def paillier_encrypt_dev(self, limbs_n: int, n, g, m, r, d_steps: int, steps_cap: int):
        """steps stay on the device (d_steps: batch x steps_cap x 4 x 2*limbs_n u64). Returns (c, ng, nr)."""
        n, g, m, r = (_np(x).reshape(-1, limbs_n) for x in (n, g, m, r))
        batch = n.shape[0]
        ng = np.zeros(batch, dtype=np.uint32)
        nr = np.zeros(batch, dtype=np.uint32)
        c = np.zeros((batch, 2 * limbs_n), dtype=np.uint64)
        self._chk(self.L.pz_paillier_encrypt_dev(self.ctx, limbs_n, batch, _ptr(n), _ptr(g), _ptr(m), _ptr(r),
                                                 VP(d_steps), steps_cap, VP(ng.ctypes.data), VP(nr.ctypes.data),
                                                 _ptr(c)), "pz_paillier_encrypt_dev")
        return c, ng, nr

    # ------------------------------------------------------------------ K3: big integers
    def mul_mod(self, limbs: int, a, b, modulus) -> Tuple[np.ndarray, np.ndarray]:
        a, b, m = (_np(x).reshape(limbs) for x in (a, b, modulus))
        q = np.zeros(limbs, dtype=np.uint64)
        r = np.zeros(limbs, dtype=np.uint64)
        self._chk(self.L.pz_mul_mod(self.ctx, limbs, _ptr(a), _ptr(b), _ptr(m), _ptr(q), _ptr(r)), "pz_mul_mod")
        return q, r

    def paillier_trace(self, limbs_n2: int, n2, base, exp, exp_limbs: int, want_steps: bool = True):
        n2, base = (_np(x).reshape(limbs_n2) for x in (n2, base))
        exp = _np(exp).reshape(exp_limbs)
        e_int = 0
        for i, l in enumerate(exp.tolist()):
            e_int |= int(l) << (64 * i)
        cap = e_int.bit_length() + bin(e_int).count("1")
        steps = np.zeros((max(cap, 1), 4, limbs_n2), dtype=np.uint64) if want_steps else None
        ns = C.c_size_t(cap)
        res = np.zeros(limbs_n2, dtype=np.uint64)
        self._chk(self.L.pz_paillier_trace(self.ctx, limbs_n2, _ptr(n2), _ptr(base), _ptr(exp), exp_limbs,
                                           _ptr(steps) if want_steps else VP(), C.byref(ns), _ptr(res)),
                  "pz_paillier_trace")
        return res, (steps[: ns.value] if want_steps else None), ns.value

    def paillier_encrypt(self, limbs_n: int, n, g, m, r, want_steps: bool = True):
        """Batch form: n, g, m, r are (batch, limbs_n).  Returns (c (batch, 2*limbs_n), steps or None,
        n_steps_g, n_steps_r)."""
        n, g, m, r = (_np(x).reshape(-1, limbs_n) for x in (n, g, m, r))
        batch = n.shape[0]
        L = 2 * limbs_n
        cap = 0
        steps = None
        if want_steps:
            for i in range(batch):
                bits = 0
                for arr in (m[i], n[i]):
                    e_int = 0
                    for k, l in enumerate(arr.tolist()):
                        e_int |= int(l) << (64 * k)
                    bits += e_int.bit_length() + bin(e_int).count("1")
                cap = max(cap, bits + 1)
            steps = np.zeros((batch, cap, 4, L), dtype=np.uint64)
        ng = np.zeros(batch, dtype=np.uint32)
        nr = np.zeros(batch, dtype=np.uint32)
        c = np.zeros((batch, L), dtype=np.uint64)
        self._chk(self.L.pz_paillier_encrypt(self.ctx, limbs_n, batch, _ptr(n), _ptr(g), _ptr(m), _ptr(r),
                                             _ptr(steps) if want_steps else VP(), cap, VP(ng.ctypes.data),
                                             VP(nr.ctypes.data), _ptr(c)), "pz_paillier_encrypt")
        return c, steps, ng, nr

    def paillier_encrypt_uniform(self, limbs_n: int, m_bits: int, n, g, m, r, want_steps: bool = True):
        """uniform-shape circuit (pz.h): batch form, 2*m_bits steps for g^m whatever the messages are.
        Returns (c, steps or None, n_steps_g, n_steps_r)."""
        n, g, m, r = (_np(x).reshape(-1, limbs_n) for x in (n, g, m, r))
        batch = n.shape[0]
        L = 2 * limbs_n
        cap, steps = 0, None
        if want_steps:
            for i in range(batch):
                e_int = 0
                for k, l in enumerate(n[i].tolist()):
                    e_int |= int(l) << (64 * k)
                cap = max(cap, 2 * m_bits + e_int.bit_length() + bin(e_int).count("1") + 1)
            steps = np.zeros((batch, cap, 4, L), dtype=np.uint64)
        ng = np.zeros(batch, dtype=np.uint32)
        nr = np.zeros(batch, dtype=np.uint32)
        c = np.zeros((batch, L), dtype=np.uint64)
        self._chk(self.L.pz_paillier_encrypt_uniform(self.ctx, limbs_n, batch, m_bits, _ptr(n), _ptr(g), _ptr(m), _ptr(r),
                                                     _ptr(steps) if want_steps else VP(), cap, VP(ng.ctypes.data), VP(nr.ctypes.data),
                                                     _ptr(c)), "pz_paillier_encrypt_uniform")
        return c, steps, ng, nr

    def paillier_encrypt_uniform_dev(self, limbs_n: int, m_bits: int, n, g, m, r, d_steps: int, steps_cap: int):
        """uniform-shape trace, steps stay on the device (d_steps: batch x steps_cap x 4 x 2*limbs_n u64). Returns (c, ng, nr)."""
        n, g, m, r = (_np(x).reshape(-1, limbs_n) for x in (n, g, m, r))
        batch = n.shape[0]
        ng = np.zeros(batch, dtype=np.uint32)
        nr = np.zeros(batch, dtype=np.uint32)
        c = np.zeros((batch, 2 * limbs_n), dtype=np.uint64)
        self._chk(self.L.pz_paillier_encrypt_uniform_dev(self.ctx, limbs_n, batch, m_bits, _ptr(n), _ptr(g), _ptr(m), _ptr(r),
                                                         VP(d_steps), steps_cap, VP(ng.ctypes.data), VP(nr.ctypes.data), _ptr(c)),
                  "pz_paillier_encrypt_uniform_dev")
        return c, ng, nr

    def paillier_tally(self, limbs_n: int, n, cts, want_steps: bool = True):
        """product tree of B full-width ciphertexts (pz.h pz_paillier_tally): cts is (B, 2*limbs_n).  Returns (C (2*limbs_n,),
        steps (B - 1, 4, 2*limbs_n) in level-major order, or None)."""
        L = 2 * limbs_n
        n = _np(n).reshape(limbs_n)
        cts = _np(cts).reshape(-1, L)
        count = cts.shape[0]
        steps = np.zeros((max(count - 1, 1), 4, L), dtype=np.uint64) if want_steps else None
        c = np.zeros(L, dtype=np.uint64)
        self._chk(self.L.pz_paillier_tally(self.ctx, limbs_n, count, _ptr(n), _ptr(cts), _ptr(steps) if want_steps else VP(),
                                           max(count - 1, 0), _ptr(c)), "pz_paillier_tally")
        return c, (steps[: count - 1] if want_steps else None)

    def paillier_tally_dev(self, limbs_n: int, n, cts, d_steps: int, steps_cap: int):
        """the same with the B - 1 records left on the device for K4 (d_steps: steps_cap x 4 x 2*limbs_n u64).  Returns C."""
        L = 2 * limbs_n
        n = _np(n).reshape(limbs_n)
        cts = _np(cts).reshape(-1, L)
        c = np.zeros(L, dtype=np.uint64)
        self._chk(self.L.pz_paillier_tally_dev(self.ctx, limbs_n, cts.shape[0], _ptr(n), _ptr(cts), VP(d_steps), steps_cap, _ptr(c)),
                  "pz_paillier_tally_dev")
        return c

    def paillier_wtally(self, limbs_n: int, n, cts, weights, w_bits: int, want_steps: bool = True):
        """prod c_i^w_i mod n^2 (pz.h pz_paillier_wtally): cts is (B, 2*limbs_n), weights B integers below 2^w_bits.  Returns
        (C (2*limbs_n,), steps (2 B w_bits + B - 1, 4, 2*limbs_n) -- the chains' records chain-major, then the tree's -- or None)."""
        L = 2 * limbs_n
        n = _np(n).reshape(limbs_n)
        cts = _np(cts).reshape(-1, L)
        wts = np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1)
        count = cts.shape[0]
        if wts.shape[0] != count:
            raise ValueError("one weight per ciphertext")
        ns = 2 * count * w_bits + count - 1
        steps = np.zeros((max(ns, 1), 4, L), dtype=np.uint64) if want_steps else None
        c = np.zeros(L, dtype=np.uint64)
        self._chk(self.L.pz_paillier_wtally(self.ctx, limbs_n, count, w_bits, _ptr(n), _ptr(cts), _ptr(wts), _ptr(steps) if want_steps else VP(),
                                            max(ns, 0), _ptr(c)), "pz_paillier_wtally")
        return c, (steps[:ns] if want_steps else None)

    def paillier_wtally_dev(self, limbs_n: int, n, cts, weights, w_bits: int, d_steps: int, steps_cap: int):
        """the same with the records left on the device for K4 (d_steps: steps_cap x 4 x 2*limbs_n u64).  Returns C."""
        L = 2 * limbs_n
        n = _np(n).reshape(limbs_n)
        cts = _np(cts).reshape(-1, L)
        wts = np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1)
        if wts.shape[0] != cts.shape[0]:
            raise ValueError("one weight per ciphertext")
        c = np.zeros(L, dtype=np.uint64)
        self._chk(self.L.pz_paillier_wtally_dev(self.ctx, limbs_n, cts.shape[0], w_bits, _ptr(n), _ptr(cts), _ptr(wts), VP(d_steps), steps_cap,
                                                _ptr(c)), "pz_paillier_wtally_dev")
        return c

    @staticmethod
    def ballot_steps_r(n) -> int:
        """records of ONE r^n chain of a ballot: bits(n) + popcount(n) (n as an integer or 64-bit words)"""
        if not isinstance(n, int):
            n = sum(int(l) << (64 * k) for k, l in enumerate(_np(n).reshape(-1).tolist()))
        return n.bit_length() + bin(n).count("1")

    def _ballot_args(self, limbs_n: int, n, g, ms, rs):
        n, g = _np(n).reshape(limbs_n), _np(g).reshape(limbs_n)
        rs = _np(rs).reshape(-1, limbs_n)
        ms = np.ascontiguousarray(ms, dtype=np.uint64).reshape(-1)
        if ms.shape[0] != rs.shape[0]:
            raise ValueError("one message and one r per ciphertext")
        return n, g, ms, rs

    def paillier_ballot(self, limbs_n: int, n, g, ms, rs, m_bits: int, want_steps: bool = True):
        """c_i = g^m_i r_i^n mod n^2 for K messages below 2^m_bits under one key (pz.h pz_paillier_ballot): ms K integers, rs
        (K, limbs_n).  Returns (c (K, 2*limbs_n), steps (K, 2 m_bits + nr + 1, 4, 2*limbs_n) or None, nr = the records of one r^n chain)."""
        L = 2 * limbs_n
        n, g, ms, rs = self._ballot_args(limbs_n, n, g, ms, rs)
        count = ms.shape[0]
        per = 2 * m_bits + self.ballot_steps_r(n) + 1
        steps = np.zeros((max(count, 1), per, 4, L), dtype=np.uint64) if want_steps else None
        c = np.zeros((max(count, 1), L), dtype=np.uint64)
        nr = C.c_uint32()
        self._chk(self.L.pz_paillier_ballot(self.ctx, limbs_n, count, m_bits, _ptr(n), _ptr(g), _ptr(ms), _ptr(rs),
                                            _ptr(steps) if want_steps else VP(), count * per, C.byref(nr), _ptr(c)), "pz_paillier_ballot")
        return c, steps, nr.value

    def paillier_ballot_dev(self, limbs_n: int, n, g, ms, rs, m_bits: int, d_steps: int, steps_cap: int):
        """the same with the records left on the device for K4 (d_steps: steps_cap x 4 x 2*limbs_n u64).  Returns (c, nr)."""
        n, g, ms, rs = self._ballot_args(limbs_n, n, g, ms, rs)
        c = np.zeros((max(ms.shape[0], 1), 2 * limbs_n), dtype=np.uint64)
        nr = C.c_uint32()
        self._chk(self.L.pz_paillier_ballot_dev(self.ctx, limbs_n, ms.shape[0], m_bits, _ptr(n), _ptr(g), _ptr(ms), _ptr(rs), VP(d_steps),
                                                steps_cap, C.byref(nr), _ptr(c)), "pz_paillier_ballot_dev")
        return c, nr.value

    # the short-randomness ballot: c_i = g^m_i hs^s_i mod n^2, hs = h^n mod n^2 from keys.djn_generator
    @staticmethod
    def _sballot_args(limbs_n: int, n, g, hs, ms, ss, s_bits: int):
        n, g, hs = _np(n).reshape(limbs_n), _np(g).reshape(limbs_n), _np(hs).reshape(2 * limbs_n)
        ms = np.ascontiguousarray(ms, dtype=np.uint64).reshape(-1)
        ss = _np(ss).reshape(-1, max(-(-s_bits // 64), 1))
        if ms.shape[0] != ss.shape[0]:
            raise ValueError("one message and one s per ciphertext")
        return n, g, hs, ms, ss

    def paillier_sballot(self, limbs_n: int, n, g, hs, ms, ss, m_bits: int, s_bits: int, want_steps: bool = True):
        """c_i = g^m_i hs^s_i mod n^2 for K messages below 2^m_bits and K exponents below 2^s_bits under one key (pz.h
        pz_paillier_sballot): hs (2*limbs_n,) words, ms K integers, ss (K, ceil(s_bits / 64)) words.  s_bits is the caller's: security
        rests on the short-exponent assumption in <hs>.  Returns (c (K, 2*limbs_n), steps (K, 2 m_bits + 2 s_bits + 1, 4, 2*limbs_n) or
        None)."""
        L = 2 * limbs_n
        n, g, hs, ms, ss = self._sballot_args(limbs_n, n, g, hs, ms, ss, s_bits)
        count = ms.shape[0]
        per = 2 * m_bits + 2 * s_bits + 1
        steps = np.zeros((max(count, 1), per, 4, L), dtype=np.uint64) if want_steps else None
        c = np.zeros((max(count, 1), L), dtype=np.uint64)
        self._chk(self.L.pz_paillier_sballot(self.ctx, limbs_n, count, m_bits, s_bits, _ptr(n), _ptr(g), _ptr(hs), _ptr(ms), _ptr(ss),
                                             _ptr(steps) if want_steps else VP(), count * per, _ptr(c)), "pz_paillier_sballot")
        return c, steps

    def paillier_sballot_dev(self, limbs_n: int, n, g, hs, ms, ss, m_bits: int, s_bits: int, d_steps: int, steps_cap: int):
        """the same with the records left on the device for K4 (d_steps: steps_cap x 4 x 2*limbs_n u64; 0: the values only).  Returns c."""
        n, g, hs, ms, ss = self._sballot_args(limbs_n, n, g, hs, ms, ss, s_bits)
        c = np.zeros((max(ms.shape[0], 1), 2 * limbs_n), dtype=np.uint64)
        self._chk(self.L.pz_paillier_sballot_dev(self.ctx, limbs_n, ms.shape[0], m_bits, s_bits, _ptr(n), _ptr(g), _ptr(hs), _ptr(ms), _ptr(ss),
                                                 VP(d_steps), steps_cap, _ptr(c)), "pz_paillier_sballot_dev")
        return c

    # the packed ballot: c_i = (prod_j G_j^v_ij) hs^s_i mod n^2, G_j = g^(2^(j w)) from keys.pballot_bases
    @staticmethod
    def _pballot_args(limbs_n: int, n, hs, gs, vs, ss, s_bits: int):
        n, hs = _np(n).reshape(limbs_n), _np(hs).reshape(2 * limbs_n)
        gs = _np(gs).reshape(-1, 2 * limbs_n)
        vs = np.ascontiguousarray(vs, dtype=np.uint64)
        vs = vs.reshape(-1, gs.shape[0]) if gs.shape[0] else vs.reshape(0, 0)
        ss = _np(ss).reshape(-1, max(-(-s_bits // 64), 1))
        if vs.shape[0] != ss.shape[0]:
            raise ValueError("one row of slot values and one s per ciphertext")
        return n, hs, gs, vs, ss

    def paillier_pballot(self, limbs_n: int, n, hs, gs, vs, ss, m_bits: int, s_bits: int, want_steps: bool = True):
        """c_i = (prod_j G_j^v_ij) hs^s_i mod n^2 for R ciphertexts of K slot values below 2^m_bits and R exponents below 2^s_bits under
        one key (pz.h pz_paillier_pballot): hs (2*limbs_n,) words, gs (K, 2*limbs_n) words (keys.pballot_bases), vs (R, K) integers, ss
        (R, ceil(s_bits / 64)) words.  Returns (c (R, 2*limbs_n), steps (R, 2 m_bits K + 2 s_bits + K, 4, 2*limbs_n) or None)."""
        L = 2 * limbs_n
        n, hs, gs, vs, ss = self._pballot_args(limbs_n, n, hs, gs, vs, ss, s_bits)
        count, slots = vs.shape
        per = 2 * m_bits * slots + 2 * s_bits + slots
        steps = np.zeros((max(count, 1), per, 4, L), dtype=np.uint64) if want_steps else None
        c = np.zeros((max(count, 1), L), dtype=np.uint64)
        self._chk(self.L.pz_paillier_pballot(self.ctx, limbs_n, count, slots, m_bits, s_bits, _ptr(n), _ptr(hs), _ptr(gs), _ptr(vs), _ptr(ss),
                                             _ptr(steps) if want_steps else VP(), count * per, _ptr(c)), "pz_paillier_pballot")
        return c, steps

    def paillier_pballot_dev(self, limbs_n: int, n, hs, gs, vs, ss, m_bits: int, s_bits: int, d_steps: int, steps_cap: int):
        """the same with the records left on the device (d_steps: steps_cap x 4 x 2*limbs_n u64; 0: the values only).  Returns c."""
        n, hs, gs, vs, ss = self._pballot_args(limbs_n, n, hs, gs, vs, ss, s_bits)
        c = np.zeros((max(vs.shape[0], 1), 2 * limbs_n), dtype=np.uint64)
        self._chk(self.L.pz_paillier_pballot_dev(self.ctx, limbs_n, vs.shape[0], vs.shape[1], m_bits, s_bits, _ptr(n), _ptr(hs), _ptr(gs),
                                                 _ptr(vs), _ptr(ss), VP(d_steps), steps_cap, _ptr(c)), "pz_paillier_pballot_dev")
        return c

    # the mix: shuffle and re-randomise K = 2^d ciphertexts under one key
    @staticmethod
    def mix_route(perm) -> np.ndarray:
        """the switch bits of a mixer's permutation (pz.h pz_mix_route; host logic, needs no context): perm[i] = the index of the input
        that output position i receives.  Returns the (2d - 1) K / 2 bytes of the Benes network, layer-major.  mix.benes_route is the
        same in Python integers."""
        perm = np.ascontiguousarray(perm, dtype=np.uint32).reshape(-1)
        count = perm.shape[0]
        d = max(count.bit_length() - 1, 0)
        bits = np.zeros(max((2 * d - 1) * (count // 2), 1), dtype=np.uint8)
        rc = _lib.lib().pz_mix_route(count, VP(perm.ctypes.data), VP(bits.ctypes.data))
        if rc != 0:
            raise PzError(rc, "pz_mix_route")
        return bits[: max(2 * d - 1, 0) * (count // 2)]

    @staticmethod
    def _mix_args(limbs_n: int, n, cts, bits, rs):
        n = _np(n).reshape(limbs_n)
        cts, rs = _np(cts).reshape(-1, 2 * limbs_n), _np(rs).reshape(-1, limbs_n)
        if cts.shape[0] != rs.shape[0]:
            raise ValueError("one r per ciphertext")
        return n, cts, np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1), rs

    @staticmethod
    def mix_layers(count: int) -> int:
        """layers of the network over count positions: 2 log2(count) - 1, none for one position"""
        return max(2 * (count.bit_length() - 1) - 1, 0)

    def paillier_mix(self, limbs_n: int, n, cts, bits, rs, want_steps: bool = True, want_routes: bool = True):
        """c'_i = c_perm(i) r_i^n mod n^2 (pz.h pz_paillier_mix): cts (K, 2*limbs_n), bits the network's switch bytes (mix_route), rs
        (K, limbs_n).  Returns (mixed (K, 2*limbs_n), routes (2d - 1, K, 2*limbs_n) or None, steps (K, nr + 1, 4, 2*limbs_n) or None)."""
        L = 2 * limbs_n
        n, cts, bits, rs = self._mix_args(limbs_n, n, cts, bits, rs)
        count = cts.shape[0]
        per = self.ballot_steps_r(n) + 1
        routes = np.zeros((max(self.mix_layers(count), 1), max(count, 1), L), dtype=np.uint64) if want_routes else None
        steps = np.zeros((max(count, 1), per, 4, L), dtype=np.uint64) if want_steps else None
        mixed = np.zeros((max(count, 1), L), dtype=np.uint64)
        self._chk(self.L.pz_paillier_mix(self.ctx, limbs_n, count, _ptr(n), _ptr(cts), VP(bits.ctypes.data), _ptr(rs),
                                         _ptr(routes) if want_routes else VP(), _ptr(steps) if want_steps else VP(), count * per,
                                         _ptr(mixed)), "pz_paillier_mix")
        return mixed, (routes[: self.mix_layers(count)] if want_routes else None), steps

    def paillier_mix_dev(self, limbs_n: int, n, cts, bits, rs, d_routes: int, d_steps: int, steps_cap: int):
        """the same with the route layers and the records left on the device (d_routes: (2d - 1) x K x 2*limbs_n u64, d_steps: steps_cap
        x 4 x 2*limbs_n u64; either may be 0).  Returns mixed."""
        n, cts, bits, rs = self._mix_args(limbs_n, n, cts, bits, rs)
        mixed = np.zeros((max(cts.shape[0], 1), 2 * limbs_n), dtype=np.uint64)
        self._chk(self.L.pz_paillier_mix_dev(self.ctx, limbs_n, cts.shape[0], _ptr(n), _ptr(cts), VP(bits.ctypes.data), _ptr(rs),
                                             VP(d_routes), VP(d_steps), steps_cap, _ptr(mixed)), "pz_paillier_mix_dev")
        return mixed

    # the short-randomness mix: c'_i = c_perm(i) hs^s_i mod n^2, hs = h^n mod n^2 from keys.djn_generator
    @staticmethod
    def _smix_args(limbs_n: int, n, hs, cts, bits, ss, s_bits: int):
        n, hs = _np(n).reshape(limbs_n), _np(hs).reshape(2 * limbs_n)
        cts, ss = _np(cts).reshape(-1, 2 * limbs_n), _np(ss).reshape(-1, max(-(-s_bits // 64), 1))
        if cts.shape[0] != ss.shape[0]:
            raise ValueError("one s per ciphertext")
        return n, hs, cts, np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1), ss

    def paillier_smix(self, limbs_n: int, n, hs, cts, bits, ss, s_bits: int, want_steps: bool = True, want_routes: bool = True):
        """c'_i = c_perm(i) hs^s_i mod n^2 for K exponents below 2^s_bits (pz.h pz_paillier_smix): hs (2*limbs_n,) words, cts (K,
        2*limbs_n), bits the network's switch bytes (mix_route), ss (K, ceil(s_bits / 64)) words.  s_bits is the caller's: hiding rests on
        the short-exponent assumption in <hs>.  Returns (mixed (K, 2*limbs_n), routes (2d - 1, K, 2*limbs_n) or None, steps (K, 2 s_bits
        + 1, 4, 2*limbs_n) or None)."""
        L = 2 * limbs_n
        n, hs, cts, bits, ss = self._smix_args(limbs_n, n, hs, cts, bits, ss, s_bits)
        count = cts.shape[0]
        per = 2 * s_bits + 1
        routes = np.zeros((max(self.mix_layers(count), 1), max(count, 1), L), dtype=np.uint64) if want_routes else None
        steps = np.zeros((max(count, 1), per, 4, L), dtype=np.uint64) if want_steps else None
        mixed = np.zeros((max(count, 1), L), dtype=np.uint64)
        self._chk(self.L.pz_paillier_smix(self.ctx, limbs_n, count, s_bits, _ptr(n), _ptr(hs), _ptr(cts), VP(bits.ctypes.data), _ptr(ss),
                                          _ptr(routes) if want_routes else VP(), _ptr(steps) if want_steps else VP(), count * per,
                                          _ptr(mixed)), "pz_paillier_smix")
        return mixed, (routes[: self.mix_layers(count)] if want_routes else None), steps

    def paillier_smix_dev(self, limbs_n: int, n, hs, cts, bits, ss, s_bits: int, d_routes: int, d_steps: int, steps_cap: int):
        """the same with the route layers and the records left on the device (d_routes: (2d - 1) x K x 2*limbs_n u64, d_steps: steps_cap
        x 4 x 2*limbs_n u64; either may be 0).  Returns mixed."""
        n, hs, cts, bits, ss = self._smix_args(limbs_n, n, hs, cts, bits, ss, s_bits)
        mixed = np.zeros((max(cts.shape[0], 1), 2 * limbs_n), dtype=np.uint64)
        self._chk(self.L.pz_paillier_smix_dev(self.ctx, limbs_n, cts.shape[0], s_bits, _ptr(n), _ptr(hs), _ptr(cts), VP(bits.ctypes.data),
                                              _ptr(ss), VP(d_routes), VP(d_steps), steps_cap, _ptr(mixed)), "pz_paillier_smix_dev")
        return mixed

    def paillier_sk(self, limbs_n: int, n, g, lam, d, p=None, q=None) -> "PaillierSecretKey":
        """a secret key handle (pz.h pz_paillier_sk_create): n, g, lambda and d = n^-1 mod lambda as integers or limbs_n-word arrays
        (keys.secret_from_primes gives all four).  The key is validated on the device; free() wipes the handle's device memory.
        With both primes p and q (pz.h pz_paillier_sk_create_crt) the handle also serves the CRT path; one without the other is an
        error."""
        return PaillierSecretKey(self, limbs_n, n, g, lam, d, p, q)

    # crt=None takes the CRT path where it is the faster one (profiles/decrypt_crt_probe.jsonl): always when n^2
    # leaves the 64-limb instantiation (limbs_n > 32), else while the 2 B half-length teams are resident at once (256 CUs x 2 teams);
    # beyond that they run in as many rounds as the lambda path's B teams take in full-length ones, and the split and Garner launches
    # are extra (2048 bits, B = 1024: 0.96 .. 0.98 of the lambda path's speed)
    CRT_AUTO_MAX_TEAMS = 512

    @classmethod
    def _use_crt(cls, sk: "PaillierSecretKey", crt, count: int) -> bool:
        """crt=False: the lambda path; True: the CRT path (an error on a handle without one); None: the CRT path where the handle has
        one and the probe found it no slower at this shape"""
        if crt is None:
            return sk.has_crt and (sk.limbs_n > 32 or 2 * count <= cls.CRT_AUTO_MAX_TEAMS)
        if crt and not sk.has_crt:
            raise PzError(_lib.PZ_ERR_INVALID, "paillier_decrypt: crt=True on a handle made without p and q")
        return bool(crt)

    def paillier_decrypt(self, sk: "PaillierSecretKey", cts, want_r: bool = True, crt=None):
        """decrypt B ciphertexts (cts: (B, 2*limbs_n) words) under sk (pz.h pz_paillier_decrypt, or pz_paillier_decrypt_crt: see
        _use_crt; the results are the same bit for bit).  Returns (m (B, limbs_n), r (B, limbs_n) or None, flags (B,) uint8: bit 0 =
        not a unit, m and r zero)."""
        Ln = sk.limbs_n
        cts = _np(cts).reshape(-1, 2 * Ln)
        count = cts.shape[0]
        m = np.zeros((count, Ln), dtype=np.uint64)
        r = np.zeros((count, Ln), dtype=np.uint64) if want_r else None
        flags = np.zeros(count, dtype=np.uint8)
        name = "pz_paillier_decrypt_crt" if self._use_crt(sk, crt, count) else "pz_paillier_decrypt"
        self._chk(getattr(self.L, name)(self.ctx, sk.handle, count, _ptr(cts), _ptr(m), _ptr(r) if want_r else VP(), VP(flags.ctypes.data)), name)
        return m, r, flags

    def paillier_decrypt_dev(self, sk: "PaillierSecretKey", count: int, d_cts: int, d_m: int, d_r: int, d_flags: int, crt=None):
        """the same on DEVICE buffers (addresses; d_r may be 0), asynchronous on the context's stream: bit 1 of a flag marks a
        ciphertext >= n^2 (pz.h pz_paillier_decrypt_dev / pz_paillier_decrypt_crt_dev)."""
        name = "pz_paillier_decrypt_crt_dev" if self._use_crt(sk, crt, count) else "pz_paillier_decrypt_dev"
        self._chk(getattr(self.L, name)(self.ctx, sk.handle, count, VP(d_cts), VP(d_m), VP(d_r) if d_r else VP(), VP(d_flags)), name)

    # T-of-T threshold decryption (pz.h pz_paillier_partial / pz_paillier_combine; keys.deal_shares deals the key)
    @staticmethod
    def partial_records(count: int, e_bits: int) -> int:
        """records of one trustee's partial decryptions: the count squarings, then count + 1 chains of 2 e_bits"""
        return count + (count + 1) * 2 * e_bits

    def _partial_args(self, limbs_n: int, n, v, theta, cts):
        L = 2 * limbs_n
        return _np(n).reshape(limbs_n), _np(v).reshape(L), _np(theta).reshape(L), _np(cts).reshape(-1, L)

    def paillier_partial(self, limbs_n: int, n, v, theta, cts, e_bits: int, want_steps: bool = True):
        """one trustee's partial decryptions h = v^theta, u_j = (c_j^2)^theta mod n^2 over exactly e_bits bits of its share theta:
        v, theta (2*limbs_n,) words, cts (K, 2*limbs_n).  Returns (h (2*limbs_n,), u (K, 2*limbs_n), steps (K + (K + 1) 2 e_bits, 4,
        2*limbs_n) or None)."""
        L = 2 * limbs_n
        n, v, theta, cts = self._partial_args(limbs_n, n, v, theta, cts)
        count = cts.shape[0]
        n_rec = self.partial_records(count, e_bits)
        steps = np.zeros((n_rec, 4, L), dtype=np.uint64) if want_steps else None
        h = np.zeros(L, dtype=np.uint64)
        u = np.zeros((max(count, 1), L), dtype=np.uint64)
        self._chk(self.L.pz_paillier_partial(self.ctx, limbs_n, count, e_bits, _ptr(n), _ptr(v), _ptr(theta), _ptr(cts),
                                             _ptr(steps) if want_steps else VP(), n_rec, _ptr(h), _ptr(u)), "pz_paillier_partial")
        return h, u, steps

    def paillier_partial_dev(self, limbs_n: int, n, v, theta, cts, e_bits: int, d_steps: int, steps_cap: int):
        """the same with the records left on the device for K4 (d_steps: steps_cap x 4 x 2*limbs_n u64).  Returns (h, u)."""
        L = 2 * limbs_n
        n, v, theta, cts = self._partial_args(limbs_n, n, v, theta, cts)
        h = np.zeros(L, dtype=np.uint64)
        u = np.zeros((max(cts.shape[0], 1), L), dtype=np.uint64)
        self._chk(self.L.pz_paillier_partial_dev(self.ctx, limbs_n, cts.shape[0], e_bits, _ptr(n), _ptr(v), _ptr(theta), _ptr(cts), VP(d_steps),
                                                 steps_cap, _ptr(h), _ptr(u)), "pz_paillier_partial_dev")
        return h, u

    def paillier_combine(self, limbs_n: int, n, mu2, partials):
        """m_j = L(prod_i u_ij mod n^2) mu2 mod n: partials (T, K, 2*limbs_n) words, trustee-major.  Returns (m (K, limbs_n), flags (K,)
        uint8: bit 0 = the product is not 1 mod n, m zero; bit 1 = a partial >= n^2: PzError PZ_ERR_RANGE, which then carries every
        entry as written in its `m` and `flags` attributes)."""
        parts = _np(partials)
        if parts.ndim != 3 or parts.shape[2] != 2 * limbs_n:
            raise ValueError("partials: (trustees, count, 2*limbs_n) words")
        trustees, count = parts.shape[0], parts.shape[1]
        n, mu2 = _np(n).reshape(limbs_n), _np(mu2).reshape(limbs_n)
        m = np.zeros((max(count, 1), limbs_n), dtype=np.uint64)
        flags = np.zeros(max(count, 1), dtype=np.uint8)
        rc = self.L.pz_paillier_combine(self.ctx, limbs_n, count, trustees, _ptr(n), _ptr(mu2), _ptr(parts), _ptr(m), VP(flags.ctypes.data))
        try:
            self._chk(rc, "pz_paillier_combine")
        except PzError as e:
            if e.status == _lib.PZ_ERR_RANGE:
                e.m, e.flags = m, flags
            raise
        return m, flags

    def paillier_combine_dev(self, limbs_n: int, n, mu2, count: int, trustees: int, d_partials: int, d_m: int, d_flags: int):
        """the same on DEVICE buffers (addresses), asynchronous on the context's stream (pz.h pz_paillier_combine_dev)"""
        n, mu2 = _np(n).reshape(limbs_n), _np(mu2).reshape(limbs_n)
        self._chk(self.L.pz_paillier_combine_dev(self.ctx, limbs_n, count, trustees, _ptr(n), _ptr(mu2), VP(d_partials), VP(d_m), VP(d_flags)),
                  "pz_paillier_combine_dev")

    # t-of-T threshold decryption with Shamir shares
    def mod_inverse(self, limbs: int, mod, xs):
        """inv_j = x_j^-1 mod `mod` for a batch under ONE odd modulus (pz.h pz_bigint_mod_inverse): mod (limbs,) words, xs (count, limbs).
        Returns (inv (count, limbs), flags (count,) uint8: bit 0 = not a unit, the output zero; bit 1 = x >= mod: PzError PZ_ERR_RANGE,
        which then carries every entry as written in its `inv` and `flags` attributes)."""
        mod, xs = _np(mod).reshape(limbs), _np(xs).reshape(-1, limbs)
        count = xs.shape[0]
        inv = np.zeros((max(count, 1), limbs), dtype=np.uint64)
        flags = np.zeros(max(count, 1), dtype=np.uint8)
        rc = self.L.pz_bigint_mod_inverse(self.ctx, limbs, count, _ptr(mod), _ptr(xs), _ptr(inv), VP(flags.ctypes.data))
        try:
            self._chk(rc, "pz_bigint_mod_inverse")
        except PzError as e:
            if e.status == _lib.PZ_ERR_RANGE:
                e.inv, e.flags = inv, flags
            raise
        return inv, flags

    def mod_inverse_dev(self, limbs: int, mod, count: int, d_xs: int, d_inv: int, d_flags: int):
        """the same on DEVICE buffers (addresses), asynchronous on the context's stream (pz.h pz_bigint_mod_inverse_dev)"""
        mod = _np(mod).reshape(limbs)
        self._chk(self.L.pz_bigint_mod_inverse_dev(self.ctx, limbs, count, _ptr(mod), VP(d_xs), VP(d_inv), VP(d_flags)),
                  "pz_bigint_mod_inverse_dev")

    # prime generation for Paillier keys
    def is_prime(self, limbs: int, cands, bases):
        """Miller-Rabin on a batch, every candidate its own modulus (pz.h pz_bigint_is_prime): cands (count, limbs) words, bases (rounds,)
        words >= 2 shared by all candidates.  Returns (flags (count,) uint8: 1 = passed every round, witness (count,) uint32: the first
        failing round, rounds if none, 0xFFFFFFFF for c < 3 and even c)."""
        cands, bases = _np(cands).reshape(-1, limbs), _np(bases).reshape(-1)
        count = cands.shape[0]
        flags = np.zeros(max(count, 1), dtype=np.uint8)
        witness = np.zeros(max(count, 1), dtype=np.uint32)
        self._chk(self.L.pz_bigint_is_prime(self.ctx, limbs, count, _ptr(cands), len(bases), _ptr(bases), VP(flags.ctypes.data),
                                            VP(witness.ctypes.data)), "pz_bigint_is_prime")
        return flags, witness

    def is_prime_dev(self, limbs: int, count: int, d_cands: int, bases, d_flags: int, d_witness: int):
        """the same on DEVICE buffers (addresses), asynchronous on the context's stream (pz.h pz_bigint_is_prime_dev)"""
        bases = _np(bases).reshape(-1)
        self._chk(self.L.pz_bigint_is_prime_dev(self.ctx, limbs, count, VP(d_cands), len(bases), _ptr(bases), VP(d_flags), VP(d_witness)),
                  "pz_bigint_is_prime_dev")

    def prime_sieve(self, limbs: int, start, window: int, safe: bool = False):
        """mask (window,) uint8 of the trial-division sieve over c_i = start + stride i (pz.h pz_prime_sieve): 1 = no odd prime below 2^16
        divides c_i (nor, with safe, (c_i - 1) / 2).  stride 2, start odd; with safe stride 4, start = 3 mod 4."""
        start = _np(start).reshape(limbs)
        mask = np.zeros(max(window, 1), dtype=np.uint8)
        self._chk(self.L.pz_prime_sieve(self.ctx, limbs, _ptr(start), window, int(safe), VP(mask.ctypes.data)), "pz_prime_sieve")
        return mask

    def prime_search(self, limbs: int, start, window: int, safe: bool, bases, want: int = 1):
        """the `want` smallest offsets i of the window whose c_i = start + stride i survives the sieve and passes every round over
        `bases` -- with safe, whose (c_i - 1) / 2 passes too (pz.h pz_prime_search).  Returns (offsets (found,) uint32 ascending,
        survivors: the sieve's count); found may be less than want, or zero."""
        start, bases = _np(start).reshape(limbs), _np(bases).reshape(-1)
        offsets = np.zeros(max(want, 1), dtype=np.uint32)
        found, survivors = C.c_uint32(0), C.c_size_t(0)
        self._chk(self.L.pz_prime_search(self.ctx, limbs, _ptr(start), window, int(safe), len(bases), _ptr(bases), want,
                                         VP(offsets.ctypes.data), C.byref(found), C.byref(survivors)), "pz_prime_search")
        return offsets[: found.value].copy(), int(survivors.value)

    @staticmethod
    def shamir_lagrange(trustees: int, ids):
        """the Lagrange exponents of a combination by the members `ids` (pz.h pz_shamir_lagrange; host logic, needs no context): returns
        (exps (members, words) uint64 magnitudes with `words` the longest one's, neg (members,) uint8 signs).  keys.lagrange_exponents is
        the same in Python integers."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        cap = 64
        exps = np.zeros((max(len(ids), 1), cap), dtype=np.uint64)
        neg = np.zeros(max(len(ids), 1), dtype=np.uint8)
        need = C.c_uint32(0)
        rc = _lib.lib().pz_shamir_lagrange(trustees, len(ids), VP(ids.ctypes.data), _ptr(exps), cap, VP(neg.ctypes.data), C.byref(need))
        if rc != 0:
            raise PzError(rc, "pz_shamir_lagrange")
        return np.ascontiguousarray(exps[:, : need.value]), neg

    @staticmethod
    def _key_words(limbs_n: int, key):
        """(n words, mu2 words, trustees) of a keys.ShamirKey or of a tuple (n, mu2, trustees) of integers or word arrays"""
        n, mu2, trustees = (key.n, key.mu2, key.trustees) if hasattr(key, "mu2") else key

        def words(x):
            if isinstance(x, int):
                if x < 0 or x >> (64 * limbs_n):
                    raise ValueError("a key value does not fit limbs_n words")
                return np.array([(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(limbs_n)], dtype=np.uint64)
            return _np(x).reshape(limbs_n)

        return words(n), words(mu2), int(trustees)

    def paillier_combine_t(self, limbs_n: int, key, ids, partials):
        """open K ciphertexts from the partials of the members `ids` (any `threshold` distinct trustee ids, 1-based) of a t-of-T key:
        key a keys.ShamirKey or (n, mu2, trustees); partials (members, K, 2*limbs_n) words in the order of ids.  The exponents come from
        pz_shamir_lagrange.  Returns (m (K, limbs_n), flags (K,) uint8: bit 0 = the partials do not belong together or are too few, bit 3
        = B mod n is no unit, m zero in both cases; bit 1 = a partial >= n^2: PzError PZ_ERR_RANGE, which then carries every entry as
        written in its `m` and `flags` attributes)."""
        parts = _np(partials)
        if parts.ndim != 3 or parts.shape[2] != 2 * limbs_n or parts.shape[0] != len(ids):
            raise ValueError("partials: (len(ids), count, 2*limbs_n) words")
        n, mu2, trustees = self._key_words(limbs_n, key)
        exps, neg = self.shamir_lagrange(trustees, ids)
        members, count = parts.shape[0], parts.shape[1]
        m = np.zeros((max(count, 1), limbs_n), dtype=np.uint64)
        flags = np.zeros(max(count, 1), dtype=np.uint8)
        rc = self.L.pz_paillier_combine_t(self.ctx, limbs_n, count, members, _ptr(n), _ptr(mu2), _ptr(exps), exps.shape[1],
                                          VP(neg.ctypes.data), _ptr(parts), _ptr(m), VP(flags.ctypes.data))
        try:
            self._chk(rc, "pz_paillier_combine_t")
        except PzError as e:
            if e.status == _lib.PZ_ERR_RANGE:
                e.m, e.flags = m, flags
            raise
        return m, flags

    def paillier_combine_t_dev(self, limbs_n: int, key, ids, count: int, d_partials: int, d_m: int, d_flags: int):
        """the same on DEVICE buffers (addresses), asynchronous on the context's stream (pz.h pz_paillier_combine_t_dev)"""
        n, mu2, trustees = self._key_words(limbs_n, key)
        exps, neg = self.shamir_lagrange(trustees, ids)
        self._chk(self.L.pz_paillier_combine_t_dev(self.ctx, limbs_n, count, len(ids), _ptr(n), _ptr(mu2), _ptr(exps), exps.shape[1],
                                                   VP(neg.ctypes.data), VP(d_partials), VP(d_m), VP(d_flags)), "pz_paillier_combine_t_dev")

    # ------------------------------------------------------------------ K4: witness expansion
    def witness_cells_per_step(self, limbs: int, limb_bits: int, lookup_bits: int) -> Tuple[int, int]:
        a = C.c_size_t()
        l = C.c_size_t()
        self._chk(self.L.pz_witness_cells_per_step(limbs, limb_bits, lookup_bits, C.byref(a), C.byref(l)),
                  "pz_witness_cells_per_step")
        return a.value, l.value

    def witness_expand(self, limbs: int, limb_bits: int, lookup_bits: int, steps, modulus, want_lookup: bool = True):
        """host form: steps (n_steps, 4, words) u64, modulus (words,) -> (advice (n_steps, cells, 4), lookup or None)"""
        st = np.ascontiguousarray(steps, dtype=np.uint64)
        n_steps = st.shape[0]
        md = np.ascontiguousarray(modulus, dtype=np.uint64)
        adv_n, lk_n = self.witness_cells_per_step(limbs, limb_bits, lookup_bits)
        adv = np.zeros((n_steps, adv_n, 4), dtype=np.uint64)
        lk = np.zeros((n_steps, lk_n, 4), dtype=np.uint64) if want_lookup else None
        self._chk(self.L.pz_witness_expand(self.ctx, limbs, limb_bits, lookup_bits, _ptr(st), n_steps, _ptr(md), _ptr(adv),
                                           _ptr(lk) if lk is not None else VP()), "pz_witness_expand")
        return adv, lk

    def witness_expand_dev(self, limbs: int, limb_bits: int, lookup_bits: int, d_steps: int, n_steps: int,
                           d_modulus: int, d_advice: int, d_lookup: int = 0):
        self._chk(self.L.pz_witness_expand_dev(self.ctx, limbs, limb_bits, lookup_bits, VP(d_steps), n_steps,
                                               VP(d_modulus), VP(d_advice), VP(d_lookup)), "pz_witness_expand_dev")

    def circuit_cells(self, kind: int, limbs_n: int, limb_bits: int, lookup_bits: int, n_steps_g: int = 0, n_steps_r: int = 0):
        a = C.c_size_t()
        l = C.c_size_t()
        self._chk(self.L.pz_circuit_cells(kind, limbs_n, limb_bits, lookup_bits, n_steps_g, n_steps_r, C.byref(a), C.byref(l)),
                  "pz_circuit_cells")
        return a.value, l.value

    def circuit_expand_dev(self, kind: int, limbs_n: int, limb_bits: int, lookup_bits: int, inputs, d_steps: int, n_steps_g: int,
                           n_steps_r: int, d_modulus: int, d_advice: int, d_lookup: int = 0, rows: int = 0, col_stride: int = 0):
        """inputs: host uint64 array n | g | x | y | res, or n | c_1 .. c_B | res for kind 3 (the tally: n_steps_g = B - 1, n_steps_r = 0;
        pz.h), or n | c_1 .. c_B | w_1 .. w_B | res for kind 4 (the weighted tally: n_steps_g = 2 B W, n_steps_r = B - 1); writes the
        whole circuit's cell stream, dense or cut into columns of `rows` cells stored `col_stride` elements apart"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        self._chk(self.L.pz_circuit_expand_dev(self.ctx, kind, limbs_n, limb_bits, lookup_bits, _ptr(inp), VP(d_steps), n_steps_g,
                                               n_steps_r, VP(d_modulus), VP(d_advice), VP(d_lookup), rows, col_stride),
                  "pz_circuit_expand_dev")

    def circuit_expand_cols_dev(self, kind: int, limbs_n: int, limb_bits: int, lookup_bits: int, inputs, d_steps: int, n_steps_g: int,
                                n_steps_r: int, d_modulus: int, d_advice: int, d_lookup: int, d_col_starts: int, n_adv_cols: int,
                                max_rows: int, lookup_rows: int, col_stride: int):
        """the whole circuit's cell stream with the advice cells in halo2-lib's break-point column layout (pz.h); d_col_starts: device
        array of n_adv_cols + 1 uint64 from layout.break_points / pz_circuit_break_points"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        self._chk(self.L.pz_circuit_expand_cols_dev(self.ctx, kind, limbs_n, limb_bits, lookup_bits, _ptr(inp), VP(d_steps), n_steps_g,
                                                    n_steps_r, VP(d_modulus), VP(d_advice), VP(d_lookup), VP(d_col_starts), n_adv_cols,
                                                    max_rows, lookup_rows, col_stride), "pz_circuit_expand_cols_dev")

    # the ballot (circuit kind 6, pz.h pz_ballot_*): its shape is (count, m_bits, n_steps_r), which the by-kind calls have no place for
    def ballot_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, m_bits: int, n_steps_r: int):
        a = C.c_size_t()
        l = C.c_size_t()
        self._chk(self.L.pz_ballot_cells(limbs_n, limb_bits, lookup_bits, count, m_bits, n_steps_r, C.byref(a), C.byref(l)), "pz_ballot_cells")
        return a.value, l.value

    def ballot_public_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, m_bits: int, n_steps_r: int):
        """stream indices of the exposed cells in statement order: n | g | c_1 .. c_K | S (K >= 2)"""
        out = np.zeros(2 * limbs_n * (count + 1) + 1, dtype=np.uint64)
        npub = C.c_size_t()
        self._chk(self.L.pz_ballot_public_cells(limbs_n, limb_bits, lookup_bits, count, m_bits, n_steps_r, _ptr(out), out.shape[0],
                                                C.byref(npub)), "pz_ballot_public_cells")
        return out[: npub.value]

    def ballot_expand_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, m_bits: int, n_steps_r: int, inputs, d_steps: int,
                          d_modulus: int, d_advice: int, d_lookup: int = 0, rows: int = 0, col_stride: int = 0):
        """inputs: host uint64 array n | g | m_1 .. m_K (one word each) | r_1 .. r_K | res_1 .. res_K; d_steps: the K (2 m_bits + n_steps_r
        + 1) records of paillier_ballot_dev; writes the ballot's cell stream, dense or cut into columns"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        self._chk(self.L.pz_ballot_expand_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, m_bits, n_steps_r, _ptr(inp), VP(d_steps),
                                              VP(d_modulus), VP(d_advice), VP(d_lookup), rows, col_stride), "pz_ballot_expand_dev")

    def ballot_expand_cols_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, m_bits: int, n_steps_r: int, inputs,
                               d_steps: int, d_modulus: int, d_advice: int, d_lookup: int, d_col_starts: int, n_adv_cols: int, max_rows: int,
                               lookup_rows: int, col_stride: int):
        """the same with the advice cells in break-point columns (circuit_expand_cols_dev's conventions)"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        self._chk(self.L.pz_ballot_expand_cols_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, m_bits, n_steps_r, _ptr(inp), VP(d_steps),
                                                   VP(d_modulus), VP(d_advice), VP(d_lookup), VP(d_col_starts), n_adv_cols, max_rows,
                                                   lookup_rows, col_stride), "pz_ballot_expand_cols_dev")

    # a trustee's partial decryptions (circuit kind 7, pz.h pz_partial_*): its shape is count and the key size alone
    def partial_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int):
        a = C.c_size_t()
        l = C.c_size_t()
        self._chk(self.L.pz_partial_cells(limbs_n, limb_bits, lookup_bits, count, C.byref(a), C.byref(l)), "pz_partial_cells")
        return a.value, l.value

    def partial_public_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int):
        """stream indices of the exposed cells in statement order: n | v | h | c_1 | u_1 | .. | c_K | u_K"""
        out = np.zeros(limbs_n + (2 + 2 * count) * 2 * limbs_n, dtype=np.uint64)
        npub = C.c_size_t()
        self._chk(self.L.pz_partial_public_cells(limbs_n, limb_bits, lookup_bits, count, _ptr(out), out.shape[0], C.byref(npub)),
                  "pz_partial_public_cells")
        return out[: npub.value]

    def partial_expand_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, inputs, d_steps: int, d_modulus: int,
                           d_advice: int, d_lookup: int = 0, rows: int = 0, col_stride: int = 0):
        """inputs: host uint64 array n | v | theta | c_1 .. c_K | h | u_1 .. u_K; d_steps: the K + (K + 1) 2 E records of
        paillier_partial_dev with e_bits = E = 2 limbs_n limb_bits; writes the circuit's cell stream, dense or cut into columns"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        self._chk(self.L.pz_partial_expand_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, _ptr(inp), VP(d_steps), VP(d_modulus),
                                               VP(d_advice), VP(d_lookup), rows, col_stride), "pz_partial_expand_dev")

    def partial_expand_cols_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, inputs, d_steps: int, d_modulus: int,
                                d_advice: int, d_lookup: int, d_col_starts: int, n_adv_cols: int, max_rows: int, lookup_rows: int,
                                col_stride: int):
        """the same with the advice cells in break-point columns (circuit_expand_cols_dev's conventions)"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        self._chk(self.L.pz_partial_expand_cols_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, _ptr(inp), VP(d_steps), VP(d_modulus),
                                                    VP(d_advice), VP(d_lookup), VP(d_col_starts), n_adv_cols, max_rows, lookup_rows,
                                                    col_stride), "pz_partial_expand_cols_dev")

    # the mix (circuit kind 8, pz.h pz_mix_*): its shape is count = 2^d and the records of one r^n chain
    def mix_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, n_steps_r: int):
        a = C.c_size_t()
        l = C.c_size_t()
        self._chk(self.L.pz_mix_cells(limbs_n, limb_bits, lookup_bits, count, n_steps_r, C.byref(a), C.byref(l)), "pz_mix_cells")
        return a.value, l.value

    def mix_public_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, n_steps_r: int):
        """stream indices of the exposed cells in statement order: n | c_1 .. c_K | c'_1 .. c'_K"""
        out = np.zeros(limbs_n + 2 * max(count, 1) * 2 * limbs_n, dtype=np.uint64)
        npub = C.c_size_t()
        self._chk(self.L.pz_mix_public_cells(limbs_n, limb_bits, lookup_bits, count, n_steps_r, _ptr(out), out.shape[0], C.byref(npub)),
                  "pz_mix_public_cells")
        return out[: npub.value]

    def mix_expand_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, n_steps_r: int, inputs, bits, d_routes: int,
                       d_steps: int, d_modulus: int, d_advice: int, d_lookup: int = 0, rows: int = 0, col_stride: int = 0):
        """inputs: host uint64 array n | c_1 .. c_K | r_1 .. r_K | res_1 .. res_K; bits: the switch bytes paillier_mix_dev took; d_routes,
        d_steps: the route layers and the K (n_steps_r + 1) records it left; writes the mix's cell stream, dense or cut into columns"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
        self._chk(self.L.pz_mix_expand_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, n_steps_r, _ptr(inp), VP(bits.ctypes.data),
                                           VP(d_routes), VP(d_steps), VP(d_modulus), VP(d_advice), VP(d_lookup), rows, col_stride),
                  "pz_mix_expand_dev")

    def mix_expand_cols_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, n_steps_r: int, inputs, bits, d_routes: int,
                            d_steps: int, d_modulus: int, d_advice: int, d_lookup: int, d_col_starts: int, n_adv_cols: int, max_rows: int,
                            lookup_rows: int, col_stride: int):
        """the same with the advice cells in break-point columns (circuit_expand_cols_dev's conventions)"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
        self._chk(self.L.pz_mix_expand_cols_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, n_steps_r, _ptr(inp), VP(bits.ctypes.data),
                                                VP(d_routes), VP(d_steps), VP(d_modulus), VP(d_advice), VP(d_lookup), VP(d_col_starts),
                                                n_adv_cols, max_rows, lookup_rows, col_stride), "pz_mix_expand_cols_dev")

    # the short-randomness ballot (circuit kind 9, pz.h pz_sballot_*): its shape is (count, m_bits, s_limbs) and the key size alone
    def sballot_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, m_bits: int, s_limbs: int):
        a = C.c_size_t()
        l = C.c_size_t()
        self._chk(self.L.pz_sballot_cells(limbs_n, limb_bits, lookup_bits, count, m_bits, s_limbs, C.byref(a), C.byref(l)), "pz_sballot_cells")
        return a.value, l.value

    def sballot_public_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, m_bits: int, s_limbs: int):
        """stream indices of the exposed cells in statement order: n | g | hs | c_1 .. c_K | S (K >= 2)"""
        out = np.zeros(2 * limbs_n * (max(count, 1) + 2) + 1, dtype=np.uint64)
        npub = C.c_size_t()
        self._chk(self.L.pz_sballot_public_cells(limbs_n, limb_bits, lookup_bits, count, m_bits, s_limbs, _ptr(out), out.shape[0],
                                                 C.byref(npub)), "pz_sballot_public_cells")
        return out[: npub.value]

    def sballot_expand_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, m_bits: int, s_limbs: int, inputs, d_steps: int,
                           d_modulus: int, d_advice: int, d_lookup: int = 0, rows: int = 0, col_stride: int = 0):
        """inputs: host uint64 array n | g | hs | m_1 .. m_K (one word each) | s_1 .. s_K | res_1 .. res_K; d_steps: the K (2 m_bits +
        2 s_limbs limb_bits + 1) records paillier_sballot_dev left; writes the circuit's cell stream, dense or cut into columns"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        self._chk(self.L.pz_sballot_expand_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, m_bits, s_limbs, _ptr(inp), VP(d_steps),
                                               VP(d_modulus), VP(d_advice), VP(d_lookup), rows, col_stride), "pz_sballot_expand_dev")

    def sballot_expand_cols_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, m_bits: int, s_limbs: int, inputs,
                                d_steps: int, d_modulus: int, d_advice: int, d_lookup: int, d_col_starts: int, n_adv_cols: int, max_rows: int,
                                lookup_rows: int, col_stride: int):
        """the same with the advice cells in break-point columns (circuit_expand_cols_dev's conventions)"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        self._chk(self.L.pz_sballot_expand_cols_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, m_bits, s_limbs, _ptr(inp), VP(d_steps),
                                                    VP(d_modulus), VP(d_advice), VP(d_lookup), VP(d_col_starts), n_adv_cols, max_rows,
                                                    lookup_rows, col_stride), "pz_sballot_expand_cols_dev")

    # the packed ballot (circuit kind 11, pz.h pz_pballot_*): its shape is (count, slots, m_bits, s_limbs) and the key size alone
    def pballot_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, slots: int, m_bits: int, s_limbs: int):
        a = C.c_size_t()
        l = C.c_size_t()
        self._chk(self.L.pz_pballot_cells(limbs_n, limb_bits, lookup_bits, count, slots, m_bits, s_limbs, C.byref(a), C.byref(l)),
                  "pz_pballot_cells")
        return a.value, l.value

    def pballot_public_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, slots: int, m_bits: int, s_limbs: int):
        """stream indices of the exposed cells in statement order: n | hs | G_0 .. G_{K-1} | c_1 .. c_R | S_1 .. S_R (K >= 2)"""
        out = np.zeros(limbs_n + 2 * limbs_n * (1 + max(slots, 1) + max(count, 1)) + max(count, 1), dtype=np.uint64)
        npub = C.c_size_t()
        self._chk(self.L.pz_pballot_public_cells(limbs_n, limb_bits, lookup_bits, count, slots, m_bits, s_limbs, _ptr(out), out.shape[0],
                                                 C.byref(npub)), "pz_pballot_public_cells")
        return out[: npub.value]

    def pballot_expand_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, slots: int, m_bits: int, s_limbs: int, inputs,
                           d_steps: int, d_modulus: int, d_advice: int, d_lookup: int = 0, rows: int = 0, col_stride: int = 0):
        """inputs: host uint64 array n | hs | G_0 .. G_{K-1} | v_11 .. v_RK (one word each) | s_1 .. s_R | res_1 .. res_R; d_steps: the
        R (2 m_bits K + 2 s_limbs limb_bits + K) records paillier_pballot_dev left; writes the circuit's cell stream, dense or cut into
        columns"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        self._chk(self.L.pz_pballot_expand_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, slots, m_bits, s_limbs, _ptr(inp), VP(d_steps),
                                               VP(d_modulus), VP(d_advice), VP(d_lookup), rows, col_stride), "pz_pballot_expand_dev")

    def pballot_expand_cols_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, slots: int, m_bits: int, s_limbs: int, inputs,
                                d_steps: int, d_modulus: int, d_advice: int, d_lookup: int, d_col_starts: int, n_adv_cols: int, max_rows: int,
                                lookup_rows: int, col_stride: int):
        """the same with the advice cells in break-point columns (circuit_expand_cols_dev's conventions)"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        self._chk(self.L.pz_pballot_expand_cols_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, slots, m_bits, s_limbs, _ptr(inp),
                                                    VP(d_steps), VP(d_modulus), VP(d_advice), VP(d_lookup), VP(d_col_starts), n_adv_cols,
                                                    max_rows, lookup_rows, col_stride), "pz_pballot_expand_cols_dev")

    # the short-randomness mix (circuit kind 10, pz.h pz_smix_*): its shape is (count = 2^d, s_limbs) and the key size alone
    def smix_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, s_limbs: int):
        a = C.c_size_t()
        l = C.c_size_t()
        self._chk(self.L.pz_smix_cells(limbs_n, limb_bits, lookup_bits, count, s_limbs, C.byref(a), C.byref(l)), "pz_smix_cells")
        return a.value, l.value

    def smix_public_cells(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, s_limbs: int):
        """stream indices of the exposed cells in statement order: n | hs | c_1 .. c_K | c'_1 .. c'_K"""
        out = np.zeros(limbs_n + (2 * max(count, 1) + 1) * 2 * limbs_n, dtype=np.uint64)
        npub = C.c_size_t()
        self._chk(self.L.pz_smix_public_cells(limbs_n, limb_bits, lookup_bits, count, s_limbs, _ptr(out), out.shape[0], C.byref(npub)),
                  "pz_smix_public_cells")
        return out[: npub.value]

    def smix_expand_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, s_limbs: int, inputs, bits, d_routes: int,
                        d_steps: int, d_modulus: int, d_advice: int, d_lookup: int = 0, rows: int = 0, col_stride: int = 0):
        """inputs: host uint64 array n | hs | c_1 .. c_K | s_1 .. s_K | res_1 .. res_K; bits: the switch bytes paillier_smix_dev took;
        d_routes, d_steps: the route layers and the K (2 s_limbs limb_bits + 1) records it left; writes the circuit's cell stream, dense
        or cut into columns"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
        self._chk(self.L.pz_smix_expand_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, s_limbs, _ptr(inp), VP(bits.ctypes.data),
                                            VP(d_routes), VP(d_steps), VP(d_modulus), VP(d_advice), VP(d_lookup), rows, col_stride),
                  "pz_smix_expand_dev")

    def smix_expand_cols_dev(self, limbs_n: int, limb_bits: int, lookup_bits: int, count: int, s_limbs: int, inputs, bits, d_routes: int,
                             d_steps: int, d_modulus: int, d_advice: int, d_lookup: int, d_col_starts: int, n_adv_cols: int, max_rows: int,
                             lookup_rows: int, col_stride: int):
        """the same with the advice cells in break-point columns (circuit_expand_cols_dev's conventions)"""
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1)
        bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
        self._chk(self.L.pz_smix_expand_cols_dev(self.ctx, limbs_n, limb_bits, lookup_bits, count, s_limbs, _ptr(inp), VP(bits.ctypes.data),
                                                 VP(d_routes), VP(d_steps), VP(d_modulus), VP(d_advice), VP(d_lookup), VP(d_col_starts),
                                                 n_adv_cols, max_rows, lookup_rows, col_stride), "pz_smix_expand_cols_dev")

    # ------------------------------------------------------------------ "next" rows: SRS setup, evaluation at a point
    def srs_setup_g1_dev(self, k: int, s, omega, d_g: int = 0, d_g_lagrange: int = 0):
        self._chk(self.L.pz_srs_setup_g1_dev(self.ctx, k, _ptr(_np(s).reshape(4)), _ptr(_np(omega).reshape(4)), VP(d_g),
                                             VP(d_g_lagrange)), "pz_srs_setup_g1_dev")

    def srs_lagrange_from_monomial_dev(self, k: int, omega_inv, n_inv, d_g: int, d_g_lagrange: int):
        self._chk(self.L.pz_srs_lagrange_from_monomial_dev(self.ctx, k, self._fr1(omega_inv), self._fr1(n_inv), VP(d_g), VP(d_g_lagrange)),
                  "pz_srs_lagrange_from_monomial_dev")

    def permutation_sigma_dev(self, d_map_col: int, d_map_row: int, m: int, k: int, omega, delta, d_sigma: int, sigma_stride_u64: int):
        self._chk(self.L.pz_permutation_sigma_dev(self.ctx, VP(d_map_col), VP(d_map_row), m, k, self._fr1(omega), self._fr1(delta),
                                                  VP(d_sigma), sigma_stride_u64), "pz_permutation_sigma_dev")

    def permutation_sigma_part_dev(self, d_map_col: int, d_map_row: int, m_total: int, col_lo: int, n_cols: int, k: int, omega, delta,
                                   d_sigma: int, sigma_stride_u64: int):
        """columns [col_lo, col_lo + n_cols) of the m_total-column permutation (the map pointers are the whole permutation's)"""
        self._chk(self.L.pz_permutation_sigma_part_dev(self.ctx, VP(d_map_col), VP(d_map_row), m_total, col_lo, n_cols, k, self._fr1(omega),
                                                       self._fr1(delta), VP(d_sigma), sigma_stride_u64), "pz_permutation_sigma_part_dev")

    def g1_commit_mask_dev(self, bases: Bases, d_mask: int, n_cols: int, n: int, mask_stride: int, d_out: int):
        """d_out[col] (Jacobian, 12 words) = the sum of the bases at the rows where the column's mask byte is non-zero (device pointers)"""
        self._chk(self.L.pz_g1_commit_mask_dev(self.ctx, bases.handle, VP(d_mask), n_cols, n, mask_stride, VP(d_out)), "pz_g1_commit_mask_dev")

    def _vk_keygen(self, fn, name, bases_lagrange: Bases, k, lookup_bits, n_adv, n_lk, sel, constants, mc, mr, tile, n_instance=0, n_public=0):
        if isinstance(constants, np.ndarray) and constants.dtype == np.uint64 and constants.ndim == 2:
            cw = np.ascontiguousarray(constants)
        else:
            cw = np.zeros((len(constants), 4), dtype=np.uint64)
            for i, v in enumerate(constants):
                v = int(v)
                for j in range(4):
                    cw[i, j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
        m = n_adv + n_lk + 1 + n_instance
        fixed, sigma = np.zeros((n_adv + 2, 8), dtype=np.uint64), np.zeros((m, 8), dtype=np.uint64)
        if n_instance:            # fn is then the _pub entry point (the callers pass it): two more arguments
            self._chk(fn(self.ctx, bases_lagrange.handle, k, lookup_bits, n_adv, n_lk, n_instance, n_public, VP(sel), _ptr(cw) if cw.size else VP(),
                         cw.shape[0], VP(mc), VP(mr), tile, _ptr(fixed), _ptr(sigma)), name)
            return fixed, sigma
        self._chk(fn(self.ctx, bases_lagrange.handle, k, lookup_bits, n_adv, n_lk, VP(sel), _ptr(cw) if cw.size else VP(), cw.shape[0], VP(mc),
                     VP(mr), tile, _ptr(fixed), _ptr(sigma)), name)
        return fixed, sigma

    def vk_keygen_dev(self, bases_lagrange: Bases, k: int, lookup_bits: int, n_adv: int, n_lk: int, d_selectors: int, constants,
                      d_map_col: int, d_map_row: int, tile: int = 64, n_instance: int = 0, n_public: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """pz_vk_keygen_dev: the verifying key's commitments (fixed (n_adv + 2, 8), sigma (m, 8), affine) from the structure's DEVICE arrays;
        constants: canonical integers (or their (n, 4) words)"""
        fn, name = (self.L.pz_vk_keygen_pub_dev, "pz_vk_keygen_pub_dev") if n_instance else (self.L.pz_vk_keygen_dev, "pz_vk_keygen_dev")
        return self._vk_keygen(fn, name, bases_lagrange, k, lookup_bits, n_adv, n_lk, d_selectors, constants,
                               d_map_col, d_map_row, tile, n_instance, n_public)

    def vk_keygen(self, bases_lagrange: Bases, k: int, lookup_bits: int, n_adv: int, n_lk: int, selectors, constants, map_col, map_row,
                  tile: int = 64, n_instance: int = 0, n_public: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """pz_vk_keygen: the same from HOST arrays (selectors uint8 [n_adv][2^k], map_col / map_row 32-bit [m][2^k]), uploaded tile by tile"""
        n, m = 1 << k, n_adv + n_lk + 1 + n_instance
        sel = np.ascontiguousarray(selectors, dtype=np.uint8)
        mc = np.ascontiguousarray(map_col).view(np.uint32)
        mr = np.ascontiguousarray(map_row).view(np.uint32)
        if sel.shape != (n_adv, n) or mc.shape != (m, n) or mr.shape != (m, n):
            raise ValueError("selectors must be [n_adv][2^k] bytes, map_col / map_row [m][2^k] 32-bit words")
        fn, name = (self.L.pz_vk_keygen_pub, "pz_vk_keygen_pub") if n_instance else (self.L.pz_vk_keygen, "pz_vk_keygen")
        return self._vk_keygen(fn, name, bases_lagrange, k, lookup_bits, n_adv, n_lk, sel.ctypes.data, constants,
                               mc.ctypes.data, mr.ctypes.data, tile, n_instance, n_public)

    def keygen_columns_dev(self, bases: Bases, d_cols: int, n_cols: int, col_stride_u64: int, k: int, log_e: int, omega_n, omega_n_inv,
                           n_inv, coset_gens, d_commit: int, d_ext: int = 0, ext_stride_u64: int = 0):
        g = _np(coset_gens).reshape(-1)
        self._chk(self.L.pz_keygen_columns_dev(self.ctx, bases.handle, VP(d_cols), n_cols, col_stride_u64, k, log_e, self._fr1(omega_n),
                                               self._fr1(omega_n_inv), self._fr1(n_inv), _ptr(g), VP(d_commit), VP(d_ext), ext_stride_u64),
                  "pz_keygen_columns_dev")

    def g1_check_dev(self, d_points: int, n: int) -> int:
        """number of points (device, affine) that are not on the curve"""
        bad = C.c_uint64()
        self._chk(self.L.pz_g1_check_dev(self.ctx, VP(d_points), n, C.byref(bad)), "pz_g1_check_dev")
        return bad.value

    # ------------------------------------------------------------------ BN254 pairing (verifier side; pz.h)
    def g2_generator(self) -> np.ndarray:
        """halo2curves' G2 generator, 16 Montgomery words (x.c0, x.c1, y.c0, y.c1)"""
        out = np.zeros(16, dtype=np.uint64)
        self._chk(self.L.pz_g2_generator(_ptr(out)), "pz_g2_generator")
        return out

    def g2_mul_dev(self, d_g2: int, d_scalars: int, n: int, d_out: int):
        """d_out[i] = [s_i] Q_i: n G2 affine points (16 words), Fr Montgomery scalars (4 words), device pointers"""
        self._chk(self.L.pz_g2_mul_dev(self.ctx, VP(d_g2), VP(d_scalars), n, VP(d_out)), "pz_g2_mul_dev")

    def pairing_dev(self, d_g1: int, d_g2: int, n: int, d_gt: int):
        """d_gt[i] = e(P_i, Q_i), 48 words each (device pointers)"""
        self._chk(self.L.pz_pairing_dev(self.ctx, VP(d_g1), VP(d_g2), n, VP(d_gt)), "pz_pairing_dev")

    def pairing_check_dev(self, d_g1: int, d_g2: int, n_checks: int, pairs_per_check: int, d_ok: int):
        """d_ok[i] (int32) = 1 if prod_j e(P_ij, Q_ij) == 1, 0 if not, -1 if an input is off its curve (device pointers)"""
        self._chk(self.L.pz_pairing_check_dev(self.ctx, VP(d_g1), VP(d_g2), n_checks, pairs_per_check, VP(d_ok)),
                  "pz_pairing_check_dev")

    def vk_create(self, k: int, blinding_factors: int, n_adv: int, n_lk: int, fixed, sigma, g0, g2, s_g2, n_instance: int = 0,
                  n_public: int = 0) -> VkHandle:
        """pz_vk_create[_pub]: fixed (n_adv + 2, 8), sigma (m, 8), g0 (8), g2 / s_g2 (16 words or 128 RawBytes each); m counts the instance
        column when n_instance = 1"""
        w16 = lambda b: np.frombuffer(bytes(b), dtype="<u8").astype(np.uint64) if isinstance(b, (bytes, bytearray)) else _np(b).reshape(16)
        f, sg, g, a, b = _np(fixed, 8), _np(sigma, 8), _np(g0).reshape(8), w16(g2), w16(s_g2)
        if f.shape[0] != n_adv + 2 or sg.shape[0] != n_adv + n_lk + 1 + n_instance:
            raise ValueError("fixed must hold n_adv + 2 points and sigma n_adv + n_lk + 1 (+ 1 with an instance column)")
        h = VP()
        if n_instance:
            self._chk(self.L.pz_vk_create_pub(self.ctx, k, blinding_factors, n_adv, n_lk, n_instance, n_public, _ptr(f), _ptr(sg), _ptr(g), _ptr(a),
                                              _ptr(b), C.byref(h)), "pz_vk_create_pub")
            return VkHandle(self, h)
        self._chk(self.L.pz_vk_create(self.ctx, k, blinding_factors, n_adv, n_lk, _ptr(f), _ptr(sg), _ptr(g), _ptr(a), _ptr(b), C.byref(h)),
                  "pz_vk_create")
        return VkHandle(self, h)

    @staticmethod
    def _instance_words(instances, B: int) -> np.ndarray:
        """B lists of public values (integers below 2^256) -> (B, L, 4) canonical words"""
        L = len(instances[0])
        if len(instances) != B or any(len(v) != L for v in instances):
            raise ValueError("one list of public values per proof, all of one length")
        w = np.zeros((B, L, 4), dtype=np.uint64)
        for i, vals in enumerate(instances):
            for j, v in enumerate(vals):
                v = int(v)
                if v < 0 or v >> 256:
                    raise ValueError("a public value must fit 256 bits")
                for q in range(4):
                    w[i, j, q] = (v >> (64 * q)) & 0xFFFFFFFFFFFFFFFF
        return w

    def verify_batch_dev(self, vk: VkHandle, proofs, seeds: Sequence[bytes], want_h: bool = False, want_ab: bool = False, instances=None):
        """pz_verify_batch[_pub]: proofs (B, vk.proof_words) in the ABI layout -> (all_ok, verdicts [bool], h_evals (B, 4) or None,
        ab_affine (B, 2, 8) or None).  instances: per proof the list of its public values (a key with an instance column)"""
        pr = _np(proofs).reshape(-1, vk.proof_words)
        B = pr.shape[0]
        if len(seeds) != B:
            raise ValueError("one seed per proof")
        offs = np.zeros(B + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(sd) for sd in seeds])
        blob = np.frombuffer(b"".join(bytes(sd) for sd in seeds) or b"\0", dtype=np.uint8)
        verd = np.zeros(B, dtype=np.int32)
        hev = np.zeros((B, 4), dtype=np.uint64) if want_h else None
        ab = np.zeros((B, 2, 8), dtype=np.uint64) if want_ab else None
        ok = C.c_int()
        if instances is not None:
            iw = self._instance_words(instances, B)
            self._chk(self.L.pz_verify_batch_pub(vk.handle, _ptr(iw), iw.shape[1], _ptr(pr), B, VP(blob.ctypes.data), _ptr(offs), VP(verd.ctypes.data),
                                                 _ptr(hev) if want_h else None, _ptr(ab) if want_ab else None, C.byref(ok)), "pz_verify_batch_pub")
            return bool(ok.value), [bool(v) for v in verd], hev, ab
        self._chk(self.L.pz_verify_batch(vk.handle, _ptr(pr), B, VP(blob.ctypes.data), _ptr(offs), VP(verd.ctypes.data),
                                         _ptr(hev) if want_h else None, _ptr(ab) if want_ab else None, C.byref(ok)), "pz_verify_batch")
        return bool(ok.value), [bool(v) for v in verd], hev, ab

    # ------------------------------------------------------------------ halo2 wire bytes (csrc/pz_wire.hip)
    def g1_compress_dev(self, d_points: int, n: int, d_bytes: int):
        self._chk(self.L.pz_g1_compress_dev(self.ctx, VP(d_points), n, VP(d_bytes)), "pz_g1_compress_dev")

    def g1_decompress_dev(self, d_bytes: int, n: int, d_points: int, d_status: int):
        self._chk(self.L.pz_g1_decompress_dev(self.ctx, VP(d_bytes), n, VP(d_points), VP(d_status)), "pz_g1_decompress_dev")

    def g1_compress(self, points) -> np.ndarray:
        """affine points (n, 8) -> (n, 32) uint8, halo2curves' compressed form"""
        pts = _np(points, 8)
        out = np.zeros((pts.shape[0], 32), dtype=np.uint8)
        self._chk(self.L.pz_g1_compress(self.ctx, _ptr(pts), pts.shape[0], VP(out.ctypes.data)), "pz_g1_compress")
        return out

    def g1_decompress(self, data) -> Tuple[np.ndarray, np.ndarray]:
        """n x 32 bytes -> (points (n, 8), status (n) int32: 0 ok, 1 not canonical, 2 not on the curve; a refused point is the identity)"""
        b = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data,
                                 dtype=np.uint8).reshape(-1, 32)
        n = b.shape[0]
        pts = np.zeros((n, 8), dtype=np.uint64)
        st = np.zeros(n, dtype=np.int32)
        bad = C.c_uint64()
        self._chk(self.L.pz_g1_decompress(self.ctx, VP(b.ctypes.data), n, _ptr(pts), VP(st.ctypes.data), C.byref(bad)), "pz_g1_decompress")
        return pts, st

    def proof_encode(self, vk: VkHandle, proofs) -> np.ndarray:
        """pz_proof_encode: proofs (B, vk.proof_words) in pz_verify_batch's layout -> (B, vk.wire_bytes) uint8"""
        pr = _np(proofs).reshape(-1, vk.proof_words)
        out = np.zeros((pr.shape[0], vk.wire_bytes), dtype=np.uint8)
        self._chk(self.L.pz_proof_encode(vk.handle, _ptr(pr), pr.shape[0], VP(out.ctypes.data)), "pz_proof_encode")
        return out

    def proof_decode(self, vk: VkHandle, data) -> Tuple[np.ndarray, np.ndarray]:
        """pz_proof_decode: (B, vk.wire_bytes) uint8 -> (words (B, vk.proof_words), status (B) int32)"""
        b = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, vk.wire_bytes)
        B = b.shape[0]
        words = np.zeros((B, vk.proof_words), dtype=np.uint64)
        st = np.zeros(B, dtype=np.int32)
        self._chk(self.L.pz_proof_decode(vk.handle, VP(b.ctypes.data), B, _ptr(words), VP(st.ctypes.data)), "pz_proof_decode")
        return words, st

    def verify_batch_bytes_dev(self, vk: VkHandle, data, seeds: Sequence[bytes], want_h: bool = False, want_ab: bool = False, instances=None):
        """pz_verify_batch_bytes: data (B, vk.wire_bytes) uint8 -> the tuple of verify_batch_dev"""
        b = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, vk.wire_bytes)
        B = b.shape[0]
        if len(seeds) != B:
            raise ValueError("one seed per proof")
        offs = np.zeros(B + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(sd) for sd in seeds])
        blob = np.frombuffer(b"".join(bytes(sd) for sd in seeds) or b"\0", dtype=np.uint8)
        verd = np.zeros(B, dtype=np.int32)
        hev = np.zeros((B, 4), dtype=np.uint64) if want_h else None
        ab = np.zeros((B, 2, 8), dtype=np.uint64) if want_ab else None
        ok = C.c_int()
        if instances is not None:
            iw = self._instance_words(instances, B)
            self._chk(self.L.pz_verify_batch_bytes_pub(vk.handle, _ptr(iw), iw.shape[1], VP(b.ctypes.data), B, VP(blob.ctypes.data), _ptr(offs),
                                                       VP(verd.ctypes.data), _ptr(hev) if want_h else None, _ptr(ab) if want_ab else None,
                                                       C.byref(ok)), "pz_verify_batch_bytes_pub")
            return bool(ok.value), [bool(v) for v in verd], hev, ab
        self._chk(self.L.pz_verify_batch_bytes(vk.handle, VP(b.ctypes.data), B, VP(blob.ctypes.data), _ptr(offs), VP(verd.ctypes.data),
                                               _ptr(hev) if want_h else None, _ptr(ab) if want_ab else None, C.byref(ok)),
                  "pz_verify_batch_bytes")
        return bool(ok.value), [bool(v) for v in verd], hev, ab

    # ------------------------------------------------------------------ ParamsKZG files (csrc/pz_params.hip, pz_params.cpp)
    def g2_compress(self, points) -> np.ndarray:
        """G2 affine points (n, 16) -> (n, 64) uint8, halo2curves' compressed form"""
        pts = _np(points, 16)
        out = np.zeros((pts.shape[0], 64), dtype=np.uint8)
        self._chk(self.L.pz_g2_compress(self.ctx, _ptr(pts), pts.shape[0], VP(out.ctypes.data)), "pz_g2_compress")
        return out

    def g2_decompress(self, data) -> Tuple[np.ndarray, np.ndarray]:
        """n x 64 bytes -> (points (n, 16), status (n) int32: 0 ok, 1 not canonical, 2 no twist point has this x; refused = the identity)"""
        b = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data,
                                 dtype=np.uint8).reshape(-1, 64)
        n = b.shape[0]
        pts = np.zeros((n, 16), dtype=np.uint64)
        st = np.zeros(n, dtype=np.int32)
        self._chk(self.L.pz_g2_decompress(self.ctx, VP(b.ctypes.data), n, _ptr(pts), VP(st.ctypes.data), None), "pz_g2_decompress")
        return pts, st

    def g2_check_dev(self, d_points: int, n: int, d_status: int):
        self._chk(self.L.pz_g2_check_dev(self.ctx, VP(d_points), n, VP(d_status)), "pz_g2_check_dev")

    def g2_check(self, points) -> np.ndarray:
        """(n, 16) -> status (n) int32: 0 in the order-r subgroup, 1 not canonical, 2 off the twist, 3 on the twist but [r]Q != O"""
        pts = _np(points, 16)
        st = np.zeros(pts.shape[0], dtype=np.int32)
        self._chk(self.L.pz_g2_check(self.ctx, _ptr(pts), pts.shape[0], VP(st.ctypes.data)), "pz_g2_check")
        return st

    def params_file_bytes(self, k: int, fmt: int) -> int:
        n = C.c_size_t()
        self._chk(self.L.pz_params_file_bytes(k, fmt, C.byref(n)), "pz_params_file_bytes")
        return n.value

    def params_decode(self, data, fmt: int) -> "ParamsHandle":
        """pz_params_decode: file bytes (bytes, or a uint8 array such as a np.memmap) -> a params object on the device.  A refused
        file raises PzError(PZ_ERR_INVALID) whose n_bad attribute is the number of bad points (0: a size or header problem)."""
        b = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        h, bad = VP(), C.c_uint64()
        rc = self.L.pz_params_decode(self.ctx, VP(b.ctypes.data), b.size, fmt, C.byref(h), C.byref(bad))
        if rc != 0:
            err = PzError(rc, "pz_params_decode", "%d bad points" % bad.value if bad.value else "")
            err.n_bad = bad.value
            raise err
        return ParamsHandle(self, h)

    def params_from_dev(self, k: int, d_g: int, d_g_lagrange: int, g2, s_g2) -> "ParamsHandle":
        """pz_params_from_dev: 2^k device points each (copied; d_g_lagrange = 0 derives it); g2 / s_g2: 16 words or 128 RawBytes"""
        w16 = lambda b: np.frombuffer(bytes(b), dtype="<u8").astype(np.uint64) if isinstance(b, (bytes, bytearray)) else _np(b).reshape(16)
        a, b = w16(g2), w16(s_g2)
        h = VP()
        self._chk(self.L.pz_params_from_dev(self.ctx, k, VP(d_g), VP(d_g_lagrange), _ptr(a), _ptr(b), C.byref(h)), "pz_params_from_dev")
        return ParamsHandle(self, h)

    def poly_eval_dev(self, d_coeffs: int, n_cols: int, col_stride_u64: int, n: int, x, d_out: int):
        self._chk(self.L.pz_poly_eval_dev(self.ctx, VP(d_coeffs), n_cols, col_stride_u64, n, _ptr(_np(x).reshape(4)),
                                          VP(d_out)), "pz_poly_eval_dev")

    def poly_eval_multi_dev(self, d_coeffs: int, n_cols: int, col_stride_u64: int, n: int, xs, d_out: int):
        """xs: (n_points, 4), n_points <= 4; d_out: (n_cols, n_points, 4) on the device"""
        x = _np(xs).reshape(-1, 4)
        self._chk(self.L.pz_poly_eval_multi_dev(self.ctx, VP(d_coeffs), n_cols, col_stride_u64, n, _ptr(x), x.shape[0], VP(d_out)),
                  "pz_poly_eval_multi_dev")

    # ------------------------------------------------------------------ "next" rows: products, quotient, openings
    def _fr1(self, x):
        """host pointer to one Fr element; the array is kept referenced until a few calls later (a temporary
        converted from a list would otherwise be freed before the C call reads it)"""
        a = _np(x).reshape(4)
        keep = self.__dict__.setdefault("_keep", [])
        keep.append(a)
        del keep[:-32]
        return _ptr(a)

    def fr_batch_invert_dev(self, d_a: int, n: int):
        self._chk(self.L.pz_fr_batch_invert_dev(self.ctx, VP(d_a), n), "pz_fr_batch_invert_dev")

    def fr_prefix_product_dev(self, d_a: int, n: int, z0, d_z: int):
        self._chk(self.L.pz_fr_prefix_product_dev(self.ctx, VP(d_a), n, self._fr1(z0), VP(d_z)), "pz_fr_prefix_product_dev")

    def permutation_product_dev(self, d_cols: int, col_stride_u64: int, d_sigma: int, sigma_stride_u64: int, m: int,
                                log_n: int, omega, beta, gamma, delta_start, delta, z0, d_z: int):
        self._chk(self.L.pz_permutation_product_dev(self.ctx, VP(d_cols), col_stride_u64, VP(d_sigma), sigma_stride_u64, m,
                                                    log_n, self._fr1(omega), self._fr1(beta), self._fr1(gamma),
                                                    self._fr1(delta_start), self._fr1(delta), self._fr1(z0), VP(d_z)),
                  "pz_permutation_product_dev")

    def lookup_permute_dev(self, d_inputs: int, n_cols: int, col_stride_u64: int, d_table: int, rows: int, value_bits: int,
                           d_perm_inputs: int, d_perm_tables: int, out_stride_u64: int):
        self._chk(self.L.pz_lookup_permute_dev(self.ctx, VP(d_inputs), n_cols, col_stride_u64, VP(d_table), rows, value_bits,
                                               VP(d_perm_inputs), VP(d_perm_tables), out_stride_u64), "pz_lookup_permute_dev")

    def lookup_product_dev(self, d_inputs: int, input_stride_u64: int, d_table: int, d_perm_inputs: int,
                           perm_input_stride_u64: int, d_perm_tables: int, perm_table_stride_u64: int, n_lookups: int, n: int,
                           beta, gamma, z0, d_z: int, z_stride_u64: int):
        self._chk(self.L.pz_lookup_product_dev(self.ctx, VP(d_inputs), input_stride_u64, VP(d_table), VP(d_perm_inputs),
                                               perm_input_stride_u64, VP(d_perm_tables), perm_table_stride_u64, n_lookups, n,
                                               self._fr1(beta), self._fr1(gamma), self._fr1(z0), VP(d_z), z_stride_u64),
                  "pz_lookup_product_dev")

    def permutation_product_sets_dev(self, d_cols: int, col_stride_u64: int, d_sigma: int, sigma_stride_u64: int, m: int,
                                     chunk_len: int, log_n: int, usable_rows: int, omega, beta, gamma, delta, d_z: int,
                                     z_stride_u64: int):
        self._chk(self.L.pz_permutation_product_sets_dev(self.ctx, VP(d_cols), col_stride_u64, VP(d_sigma), sigma_stride_u64, m,
                                                         chunk_len, log_n, usable_rows, self._fr1(omega), self._fr1(beta),
                                                         self._fr1(gamma), self._fr1(delta), VP(d_z), z_stride_u64),
                  "pz_permutation_product_sets_dev")

    def quotient_gate_dev(self, d_adv_ext: int, adv_stride_u64: int, d_sel_ext: int, sel_stride_u64: int, n_cols: int,
                          log_ext: int, rot_step: int, y, d_h: int):
        self._chk(self.L.pz_quotient_gate_dev(self.ctx, VP(d_adv_ext), adv_stride_u64, VP(d_sel_ext), sel_stride_u64,
                                              n_cols, log_ext, rot_step, self._fr1(y), VP(d_h)), "pz_quotient_gate_dev")

    def quotient_permutation_dev(self, d_cols_ext: int, col_stride_u64: int, d_sigma_ext: int, sigma_stride_u64: int,
                                 d_z_ext: int, z_stride_u64: int, n_sets: int, chunk_len: int, m_total: int, log_ext: int,
                                 rot_step: int, last_rotation: int, d_l0: int, d_l_last: int, d_l_active: int, beta, gamma,
                                 delta, coset_g, omega_ext, y, d_h: int):
        self._chk(self.L.pz_quotient_permutation_dev(
            self.ctx, VP(d_cols_ext), col_stride_u64, VP(d_sigma_ext), sigma_stride_u64, VP(d_z_ext), z_stride_u64, n_sets,
            chunk_len, m_total, log_ext, rot_step, last_rotation, VP(d_l0), VP(d_l_last), VP(d_l_active), self._fr1(beta),
            self._fr1(gamma), self._fr1(delta), self._fr1(coset_g), self._fr1(omega_ext), self._fr1(y), VP(d_h)),
            "pz_quotient_permutation_dev")

    def quotient_permutation_part_dev(self, d_cols_ext: int, col_stride_u64: int, d_sigma_ext: int, sigma_stride_u64: int, d_z_ext: int,
                                      z_stride_u64: int, n_sets_total: int, set_lo: int, n_sets: int, chunk_len: int, m_cols: int,
                                      head: bool, log_ext: int, rot_step: int, last_rotation: int, d_l0: int, d_l_last: int,
                                      d_l_active: int, beta, gamma, delta, coset_g, omega_ext, y, d_h: int):
        """the permutation lines of evaluate_h for the sets [set_lo, set_lo + n_sets) (pz.h): tiles of extended columns in order"""
        self._chk(self.L.pz_quotient_permutation_part_dev(
            self.ctx, VP(d_cols_ext), col_stride_u64, VP(d_sigma_ext), sigma_stride_u64, VP(d_z_ext), z_stride_u64, n_sets_total, set_lo,
            n_sets, chunk_len, m_cols, int(head), log_ext, rot_step, last_rotation, VP(d_l0), VP(d_l_last), VP(d_l_active),
            self._fr1(beta), self._fr1(gamma), self._fr1(delta), self._fr1(coset_g), self._fr1(omega_ext), self._fr1(y), VP(d_h)),
            "pz_quotient_permutation_part_dev")

    def quotient_lookup_dev(self, d_input_ext: int, input_stride_u64: int, d_table_ext: int, d_perm_input_ext: int,
                            perm_input_stride_u64: int, d_perm_table_ext: int, perm_table_stride_u64: int, d_z_ext: int,
                            z_stride_u64: int, n_lookups: int, log_ext: int, rot_step: int, d_l0: int, d_l_last: int,
                            d_l_active: int, beta, gamma, y, d_h: int):
        self._chk(self.L.pz_quotient_lookup_dev(
            self.ctx, VP(d_input_ext), input_stride_u64, VP(d_table_ext), VP(d_perm_input_ext), perm_input_stride_u64,
            VP(d_perm_table_ext), perm_table_stride_u64, VP(d_z_ext), z_stride_u64, n_lookups, log_ext, rot_step, VP(d_l0),
            VP(d_l_last), VP(d_l_active), self._fr1(beta), self._fr1(gamma), self._fr1(y), VP(d_h)), "pz_quotient_lookup_dev")

    def quotient_permutation_split_dev(self, d_cols_ext: int, col_stride_u64: int, d_sigma_ext: int, sigma_stride_u64: int, d_z_ext: int,
                                       z_stride_u64: int, n_sets_total: int, set_lo: int, n_sets: int, chunk_len: int, m_cols: int,
                                       head: bool, log_ext: int, rot_step: int, last_rotation: int, d_l0: int, d_l_last: int,
                                       beta, gamma, delta, coset_g, omega_ext, y, d_h_low: int, d_h_d: int):
        """quotient_permutation_part_dev with the sets' product lines in a second accumulator, without l_active (pz.h)"""
        self._chk(self.L.pz_quotient_permutation_split_dev(
            self.ctx, VP(d_cols_ext), col_stride_u64, VP(d_sigma_ext), sigma_stride_u64, VP(d_z_ext), z_stride_u64, n_sets_total, set_lo,
            n_sets, chunk_len, m_cols, int(head), log_ext, rot_step, last_rotation, VP(d_l0), VP(d_l_last),
            self._fr1(beta), self._fr1(gamma), self._fr1(delta), self._fr1(coset_g), self._fr1(omega_ext), self._fr1(y), VP(d_h_low),
            VP(d_h_d)), "pz_quotient_permutation_split_dev")

    def quotient_lookup_split_dev(self, d_input_ext: int, input_stride_u64: int, d_table_ext: int, d_perm_input_ext: int,
                                  perm_input_stride_u64: int, d_perm_table_ext: int, perm_table_stride_u64: int, d_z_ext: int,
                                  z_stride_u64: int, n_lookups: int, log_ext: int, rot_step: int, d_l0: int, d_l_last: int,
                                  d_l_active: int, beta, gamma, y, d_h_low: int, d_h_d: int):
        """quotient_lookup_dev with each lookup's product line in a second accumulator, without l_active (pz.h)"""
        self._chk(self.L.pz_quotient_lookup_split_dev(
            self.ctx, VP(d_input_ext), input_stride_u64, VP(d_table_ext), VP(d_perm_input_ext), perm_input_stride_u64,
            VP(d_perm_table_ext), perm_table_stride_u64, VP(d_z_ext), z_stride_u64, n_lookups, log_ext, rot_step, VP(d_l0),
            VP(d_l_last), VP(d_l_active), self._fr1(beta), self._fr1(gamma), self._fr1(y), VP(d_h_low), VP(d_h_d)),
            "pz_quotient_lookup_split_dev")

    def quotient_d_rows_dev(self, d_cols: int, col_stride_u64: int, d_sigma: int, sigma_stride_u64: int, d_z: int, z_stride_u64: int,
                            m: int, chunk_len: int, d_input: int, input_stride_u64: int, d_table: int, d_perm_input: int,
                            perm_input_stride_u64: int, d_perm_table: int, perm_table_stride_u64: int, d_zl: int, zl_stride_u64: int,
                            n_lookups: int, log_n: int, row_lo: int, omega, beta, gamma, delta, y, d_out: int):
        """the product lines' weighted sum D on rows [row_lo, 2^log_n) of the domain, from the Lagrange forms (pz.h)"""
        self._chk(self.L.pz_quotient_d_rows_dev(
            self.ctx, VP(d_cols), col_stride_u64, VP(d_sigma), sigma_stride_u64, VP(d_z), z_stride_u64, m, chunk_len, VP(d_input),
            input_stride_u64, VP(d_table), VP(d_perm_input), perm_input_stride_u64, VP(d_perm_table), perm_table_stride_u64, VP(d_zl),
            zl_stride_u64, n_lookups, log_n, row_lo, self._fr1(omega), self._fr1(beta), self._fr1(gamma), self._fr1(delta),
            self._fr1(y), VP(d_out)), "pz_quotient_d_rows_dev")

    def fr_mul_row_dev(self, d_a: int, n_cols: int, col_stride_u64: int, n: int, d_row: int, d_out: int, out_stride_u64: int):
        self._chk(self.L.pz_fr_mul_row_dev(self.ctx, VP(d_a), n_cols, col_stride_u64, n, VP(d_row), VP(d_out), out_stride_u64),
                  "pz_fr_mul_row_dev")

    def quotient_finish_dev(self, d_h: int, log_n: int, log_e: int, coset_g, omega_ext):
        self._chk(self.L.pz_quotient_finish_dev(self.ctx, VP(d_h), log_n, log_e, self._fr1(coset_g), self._fr1(omega_ext)),
                  "pz_quotient_finish_dev")

    def fr_distribute_powers_dev(self, d_a: int, n_cols: int, col_stride_u64: int, n: int, g, c=None):
        self._chk(self.L.pz_fr_distribute_powers_dev(self.ctx, VP(d_a), n_cols, col_stride_u64, n, self._fr1(g),
                                                     self._fr1(c) if c is not None else None),
                  "pz_fr_distribute_powers_dev")

    def fr_lincomb_dev(self, d_polys: int, n_cols: int, col_stride_u64: int, n: int, v, d_out: int, accumulate: bool = False):
        self._chk(self.L.pz_fr_lincomb_dev(self.ctx, VP(d_polys), n_cols, col_stride_u64, n, self._fr1(v), VP(d_out),
                                           int(accumulate)), "pz_fr_lincomb_dev")

    def poly_div_linear_dev(self, d_coeffs: int, n_cols: int, col_stride_u64: int, n: int, x, d_q: int, q_stride_u64: int):
        self._chk(self.L.pz_poly_div_linear_dev(self.ctx, VP(d_coeffs), n_cols, col_stride_u64, n, self._fr1(x), VP(d_q),
                                                q_stride_u64), "pz_poly_div_linear_dev")

    def shplonk_begin_dev(self, n: int, sets, points, y, v, d_h: int):
        """sets: list of (list of device pointers, list of point indices, evals array (n_polys, n_points, 4)); points: (T, 4).
        Returns the opaque state for shplonk_finish_dev."""
        n_sets = len(sets)
        npol = (C.c_uint32 * n_sets)(*[len(s_[0]) for s_ in sets])
        npts = (C.c_uint32 * n_sets)(*[len(s_[1]) for s_ in sets])
        ptrs = [p for s_ in sets for p in s_[0]]
        parr = (VP * len(ptrs))(*[VP(p) for p in ptrs])
        idx = [i for s_ in sets for i in s_[1]]
        iarr = (C.c_uint32 * len(idx))(*idx)
        pts = _np(points, 4)
        ev = np.ascontiguousarray(np.concatenate([_np(s_[2]).reshape(-1, 4) for s_ in sets]), dtype=np.uint64)
        st = VP()
        self._chk(self.L.pz_shplonk_begin_dev(self.ctx, n, n_sets, npol, parr, npts, iarr, pts.shape[0], _ptr(pts), _ptr(ev), self._fr1(y),
                                              self._fr1(v), VP(d_h), C.byref(st)), "pz_shplonk_begin_dev")
        return st

    def shplonk_finish_dev(self, state, u, d_h: int, d_h2: int):
        self._chk(self.L.pz_shplonk_finish_dev(self.ctx, state, self._fr1(u), VP(d_h), VP(d_h2)), "pz_shplonk_finish_dev")

    # ------------------------------------------------------------------ measurement
    def timing_enable(self, on: bool = True):
        self._chk(self.L.pz_timing_enable(self.ctx, int(on)), "pz_timing_enable")

    def timing_reset(self):
        self._chk(self.L.pz_timing_reset(self.ctx), "pz_timing_reset")

    def timing_get(self, which: int) -> Tuple[float, int]:
        ms = C.c_double()
        n = C.c_uint64()
        self._chk(self.L.pz_timing_get(self.ctx, which, C.byref(ms), C.byref(n)), "pz_timing_get")
        return ms.value, n.value

    # ------------------------------------------------------------------ device memory / context ordering (plain-pointer hosts)
    def dev_alloc(self, nbytes: int) -> int:
        d = VP()
        self._chk(self.L.pz_dev_alloc(self.ctx, nbytes, C.byref(d)), "pz_dev_alloc")
        return d.value or 0

    def dev_free(self, d: int):
        self._chk(self.L.pz_dev_free(self.ctx, VP(d)), "pz_dev_free")

    def dev_arena(self, nbytes: int):
        """pz_dev_arena: reserve one block this context's later allocations (pz_dev_alloc and the library's own buffers) are carved from;
        0 releases it"""
        self._chk(self.L.pz_dev_arena(self.ctx, C.c_size_t(nbytes)), "pz_dev_arena")

    def dev_arena_info(self) -> dict:
        out = (C.c_uint64 * 6)()
        self._chk(self.L.pz_dev_arena_info(self.ctx, out), "pz_dev_arena_info")
        return dict(zip(("bytes", "used", "peak", "largest_hole", "served", "missed"), (int(v) for v in out)))

    def dev_mem_info(self):
        """-> (free, total) bytes as the driver reports them"""
        f, t = C.c_size_t(0), C.c_size_t(0)
        self._chk(self.L.pz_dev_mem_info(self.ctx, C.byref(f), C.byref(t)), "pz_dev_mem_info")
        return int(f.value), int(t.value)

    def upload(self, d_dst: int, arr):
        a = np.ascontiguousarray(arr)
        self._chk(self.L.pz_upload(self.ctx, VP(d_dst), VP(a.ctypes.data), a.nbytes), "pz_upload")

    def download(self, d_src: int, shape, dtype=np.uint64) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        self._chk(self.L.pz_download(self.ctx, VP(out.ctypes.data), VP(d_src), out.nbytes), "pz_download")
        return out

    def dev_memset(self, d: int, value: int, nbytes: int):
        self._chk(self.L.pz_dev_memset(self.ctx, VP(d), value, nbytes), "pz_dev_memset")

    def dev_copy(self, d_dst: int, d_src: int, nbytes: int):
        self._chk(self.L.pz_dev_copy(self.ctx, VP(d_dst), VP(d_src), nbytes), "pz_dev_copy")

    def dev_copy_2d(self, d_dst: int, dst_pitch: int, d_src: int, src_pitch: int, width: int, rows: int):
        """`rows` runs of `width` bytes, the runs dst_pitch / src_pitch bytes apart (device to device, on the context's stream)"""
        self._chk(self.L.pz_dev_copy_2d(self.ctx, VP(d_dst), dst_pitch, VP(d_src), src_pitch, width, rows), "pz_dev_copy_2d")

    def wait_for(self, other: "Engine"):
        """everything `other` has queued so far happens before what this engine queues from now on"""
        self._chk(self.L.pz_ctx_wait(self.ctx, other.ctx), "pz_ctx_wait")


T_MSM_ACC, T_NTT, T_TRACE, T_EXPAND, T_MSM_ALL, T_MSM_SORT, T_MSM_TREE = 0, 1, 2, 3, 4, 5, 6


class PaillierSecretKey:
    """pz_paillier_sk: lambda, d and mu live on the device; free() overwrites them before the memory is released"""

    def __init__(self, eng: "Engine", limbs_n: int, n, g, lam, d, p=None, q=None):
        def words(x):
            if isinstance(x, int):
                if x < 0 or x >> (64 * limbs_n):
                    raise ValueError("a key value does not fit limbs_n words")
                return np.array([(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(limbs_n)], dtype=np.uint64)
            return _np(x).reshape(limbs_n)

        if (p is None) != (q is None):
            raise ValueError("a CRT handle takes both primes: p and q, or neither")
        self.eng, self.limbs_n = eng, limbs_n
        self.handle = VP()
        a = [words(x) for x in ((n, g, lam, d) if p is None else (n, g, lam, d, p, q))]
        name = "pz_paillier_sk_create" if p is None else "pz_paillier_sk_create_crt"
        eng._chk(getattr(eng.L, name)(eng.ctx, limbs_n, *[_ptr(x) for x in a], C.byref(self.handle)), name)

    @property
    def has_crt(self) -> bool:
        """the handle holds the CRT part (pz.h pz_paillier_sk_has_crt)"""
        return bool(self.handle) and self.eng.L.pz_paillier_sk_has_crt(self.handle) == 1

    def params(self):
        """(mu, ginv) as integers: mu = L(g^lambda mod n^2)^-1 mod n, ginv = g^-1 mod n"""
        mu = np.zeros(self.limbs_n, dtype=np.uint64)
        gi = np.zeros(self.limbs_n, dtype=np.uint64)
        self.eng._chk(self.eng.L.pz_paillier_sk_params(self.handle, _ptr(mu), _ptr(gi)), "pz_paillier_sk_params")
        to_int = lambda a: sum(int(v) << (64 * i) for i, v in enumerate(a.tolist()))
        return to_int(mu), to_int(gi)

    def free(self):
        if self.handle:
            self.eng._chk(self.eng.L.pz_paillier_sk_free(self.eng.ctx, self.handle), "pz_paillier_sk_free")
            self.handle = VP()
