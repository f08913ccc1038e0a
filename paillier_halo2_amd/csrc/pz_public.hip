// pz_public.hip -- PUBLIC INPUTS: one optional instance column (halo2-lib's assigned_instances / num_instance_columns [D]) as the LAST
// column of the permutation, [advice | lookup advice | constants | instance].  Row i < L of it holds public value i, every other row is
// zero (halo2 does not blind instance columns); it is neither committed nor opened: the verifier evaluates it itself,
//     inst(x) = sum_{i<L} v_i l_i(x),   l_i(x) = (x^n - 1)/n  omega^i / (x - omega^i),
// and uses that as the last permuted value of the constraint expression.  DESIGN.md section 15.5.
//
// What lives here:
//   k_instance_eval / k_instance_finish   B proofs x L values -> B field elements (the verifier's side)
//   k_public_pos / k_public_find / k_public_link   pz_structure_expose: the L exposed advice cells of the reference's circuits get their
//                                          (column, row) through the break-point table and the instance cells join their copy cycles
//   k_public_gather                        a prover reads the statement off its own witness columns
// Fr arithmetic: fp.cuh only.  Workgroups of 256 lanes; the field is exact, so no lane count or tree shape changes a result.
#include <algorithm>

#include "fp.cuh"
#include "pz_internal.h"

namespace {

constexpr unsigned IT = 256;   // lanes of a workgroup
constexpr unsigned IE = 4;     // terms per lane: a workgroup covers IT * IE = 1024 rows of the instance column

struct W4 {
    uint64_t w[4];
};
__device__ __forceinline__ Fr fr_of(const W4& a) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r.v[2 * i] = (u32)a.w[i];
        r.v[2 * i + 1] = (u32)(a.w[i] >> 32);
    }
    return r;
}
__device__ __forceinline__ Fr ld(const uint64_t* p) { return fp_load<FrTag>(p); }
__device__ Fr pow_u64(Fr b, uint64_t e) {
    Fr acc = fp_one<FrTag>();
    while (e) {
        if (e & 1) acc = fp_mul(acc, b);
        b = fp_sqr(b);
        e >>= 1;
    }
    return acc;
}

// Workgroup (c, p): the terms v_i omega^i / (x_p - omega^i) of rows i in [1024 c, 1024 (c + 1)) of proof p, summed.  All denominators of
// the workgroup are inverted with ONE field inversion: lane products, an inclusive prefix and suffix scan of them over the lanes, the
// inverse of the total by lane 0, then every lane's own share inv(total) * prefix[t - 1] * suffix[t + 1] unrolled over its IE terms.
// A zero denominator (x on the domain) is replaced by one and flagged; rows >= L contribute the factor one and the term zero.
__global__ __launch_bounds__(256) void k_instance_eval(const uint64_t* __restrict__ inst, size_t L, const uint64_t* __restrict__ xs, size_t x_stride,
                                                       W4 omega_w, uint64_t* __restrict__ partial, int32_t* __restrict__ flags) {
    __shared__ Fr s_pre[IT], s_suf[IT];
    __shared__ Fr s_inv;
    const unsigned t = threadIdx.x, p = blockIdx.y;
    const size_t base = ((size_t)blockIdx.x * IT + t) * IE;
    const Fr one = fp_one<FrTag>(), omega = fr_of(omega_w), x = ld(xs + (size_t)p * x_stride);
    const uint64_t* v = inst + (size_t)p * L * 4;
    Fr wi = pow_u64(omega, base);
    Fr num[IE], den[IE], pre[IE];
    Fr prod = one;
    int fl = 0;
#pragma unroll
    for (unsigned j = 0; j < IE; ++j) {
        const size_t i = base + j;
        pre[j] = prod;
        if (i < L) {
            const Fr vi = ld(v + 4 * i);
            u32 tmp[8];
            if (!fp_sub_p(tmp, vi)) fl |= 2;   // a value >= r is no field element
            Fr d = fp_sub(x, wi);
            if (fp_is_zero(d)) {
                fl |= 1;
                d = one;
            }
            num[j] = fp_mul(fp_to_mont(vi), wi);
            den[j] = d;
            prod = fp_mul(prod, d);
        } else {
            num[j] = fp_zero<FrTag>();
            den[j] = one;
        }
        wi = fp_mul(wi, omega);
    }
    s_pre[t] = prod;
    s_suf[t] = prod;
    __syncthreads();
    for (unsigned off = 1; off < IT; off <<= 1) {
        const Fr a = s_pre[t], b = s_suf[t];
        const Fr al = t >= off ? s_pre[t - off] : one, br = t + off < IT ? s_suf[t + off] : one;
        __syncthreads();
        s_pre[t] = fp_mul(a, al);
        s_suf[t] = fp_mul(b, br);
        __syncthreads();
    }
    if (t == 0) s_inv = fp_inv(s_pre[IT - 1]);   // (never zero: zero denominators were replaced)
    __syncthreads();
    Fr run = s_inv;
    if (t > 0) run = fp_mul(run, s_pre[t - 1]);
    if (t + 1 < IT) run = fp_mul(run, s_suf[t + 1]);
    // run = 1 / (den[0] ... den[IE - 1]) of this lane
    Fr sum = fp_zero<FrTag>();
#pragma unroll
    for (int j = IE - 1; j >= 0; --j) {
        sum = fp_add(sum, fp_mul(num[j], fp_mul(run, pre[j])));
        run = fp_mul(run, den[j]);
    }
    __syncthreads();
    s_pre[t] = sum;
    __syncthreads();
    for (unsigned off = IT / 2; off > 0; off >>= 1) {
        if (t < off) s_pre[t] = fp_add(s_pre[t], s_pre[t + off]);
        __syncthreads();
    }
    if (t == 0) fp_store(partial + 4 * ((size_t)p * gridDim.x + blockIdx.x), s_pre[0]);
    if (fl) atomicOr(flags + p, fl);
}

// one lane per proof: the workgroups' partial sums, scaled by (x^n - 1)/n.  x^n = 1 (x on the domain, whatever L is) is flagged too.
__global__ __launch_bounds__(64) void k_instance_finish(const uint64_t* __restrict__ partial, unsigned n_chunks, size_t B, const uint64_t* __restrict__ xs,
                                                        size_t x_stride, unsigned k, W4 n_inv_w, uint64_t* __restrict__ out, size_t out_stride,
                                                        int32_t* __restrict__ flags) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    Fr sum = fp_zero<FrTag>();
    for (unsigned c = 0; c < n_chunks; ++c) sum = fp_add(sum, ld(partial + 4 * (p * n_chunks + c)));
    Fr xn = ld(xs + p * x_stride);
    for (unsigned i = 0; i < k; ++i) xn = fp_sqr(xn);
    const Fr z = fp_sub(xn, fp_one<FrTag>());
    if (fp_is_zero(z)) atomicOr(flags + p, 1);
    fp_store(out + p * out_stride, fp_mul(sum, fp_mul(z, fr_of(n_inv_w))));
}

// stream index of an advice cell -> (column, row): the column whose start is the last one <= c among the FILLED columns (a shared break
// cell: row 0 of the later column) -- cell_pos of pz_structure.hip
__global__ __launch_bounds__(64) void k_public_pos(const uint64_t* __restrict__ cells, size_t L, const uint64_t* __restrict__ starts, int n_used,
                                                   uint32_t* __restrict__ cell_col, uint32_t* __restrict__ cell_row) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    const uint64_t c = cells[i];
    int lo = 0, hi = n_used;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= c) lo = mid;
        else hi = mid;
    }
    cell_col[i] = (uint32_t)lo;
    cell_row[i] = (uint32_t)(c - starts[lo]);
}

// A class is a cycle in increasing (column, row) order, its last cell mapping to its first.  From exposed cell i follow the map to the
// class's LAST cell e_i (the one whose image is not greater than itself) and its first cell f_i.  Reads the m-column maps only.
__global__ __launch_bounds__(64) void k_public_find(const uint32_t* __restrict__ map_col, const uint32_t* __restrict__ map_row, uint64_t n, uint64_t cells,
                                                    const uint32_t* __restrict__ cell_col, const uint32_t* __restrict__ cell_row, size_t L,
                                                    uint64_t* __restrict__ e_out, uint64_t* __restrict__ f_out, unsigned* __restrict__ err) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    uint64_t cur = (uint64_t)cell_col[i] * n + cell_row[i], nxt = cur;
    bool found = false;
    for (uint64_t step = 0; step <= cells && cur < cells; ++step) {
        nxt = (uint64_t)map_col[cur] * n + map_row[cur];
        if (nxt <= cur) {
            found = true;
            break;
        }
        cur = nxt;
    }
    if (!found) {   // not a cycle of this convention (or a cell outside the map): nothing is linked
        *err = 1;
        cur = nxt = 0;
    }
    e_out[i] = cur;
    f_out[i] = nxt;
}

// column m of the (m + 1)-column maps.  Row r >= L: identity.  Row i < L, the instance cell (m, i), is the greatest cell of its class: the
// class's former last cell maps to it and it maps to the class's first.  Exposed cells that share a class (equal e) chain in row order.
// link[2 r] is the next row of r's class (LINK_NONE: r is its last), link[2 r + 1] is nonzero where an earlier row shares the class:
// class_links groups the rows by e on the host, so a lane reads its own two words and a tally's tens of thousands of cells cost O(L).
constexpr uint32_t LINK_NONE = 0xffffffffu;
__global__ __launch_bounds__(256) void k_public_link(uint32_t* __restrict__ map_col, uint32_t* __restrict__ map_row, uint64_t n, uint32_t m, size_t L,
                                                     const uint64_t* __restrict__ e, const uint64_t* __restrict__ f, const uint32_t* __restrict__ link) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint64_t self = (uint64_t)m * n + r;
    if (r >= L) {
        map_col[self] = m;
        map_row[self] = (uint32_t)r;
        return;
    }
    const uint32_t next = link[2 * r];
    if (next != LINK_NONE) {
        map_col[self] = m;
        map_row[self] = next;
    } else {
        map_col[self] = (uint32_t)(f[r] / n);
        map_row[self] = (uint32_t)(f[r] % n);
    }
    if (!link[2 * r + 1]) {
        const uint64_t ei = e[r];
        map_col[ei] = m;
        map_row[ei] = (uint32_t)r;
    }
}

// the rows of each class (equal e) in increasing order: a sort of the L row numbers by (e, row)
void class_links(const std::vector<uint64_t>& e, std::vector<uint32_t>& link) {
    const size_t L = e.size();
    std::vector<uint32_t> order(L);
    for (size_t i = 0; i < L; ++i) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return e[a] != e[b] ? e[a] < e[b] : a < b; });
    link.assign(2 * L, 0);
    for (size_t i = 0; i < L; ++i) {
        const uint32_t r = order[i];
        link[2 * r] = i + 1 < L && e[order[i + 1]] == e[r] ? order[i + 1] : LINK_NONE;
        link[2 * r + 1] = i > 0 && e[order[i - 1]] == e[r];
    }
}

// the exposed cells of a witness column block (Montgomery) as canonical words
__global__ __launch_bounds__(64) void k_public_gather(const uint64_t* __restrict__ cols, size_t col_stride, const uint32_t* __restrict__ cell_col,
                                                      const uint32_t* __restrict__ cell_row, size_t L, uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    fp_store(out + 4 * i, fp_from_mont(ld(cols + (size_t)cell_col[i] * col_stride + 4ull * cell_row[i])));
}

W4 w4_of(const uint64_t v[4]) { return W4{{v[0], v[1], v[2], v[3]}}; }

// stream indices of the exposed cells: n | g | c (encrypt, encrypt_uniform) or n | g | c1 | c2 | c (add), little-endian limbs.  The four
// assign_integer at the head of the stream put their limbs_n limb cells first; res is the assign_integer(2 limbs_n) in front of the final
// assert_equal_fresh, the last two operations of the stream.  Tally (kind 3, n_steps_g + 1 ciphertexts): n | c_1 | .. | c_B | C, the
// ciphertexts' 2 limbs_n limb cells at the head of their assign_integer blocks, which follow n's.  Decrypt (kind 5): n | g | m | c.
int public_cells(int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t n_steps_g, size_t n_steps_r, std::vector<uint64_t>& cells) {
    if (kind < 0 || kind > 5 || limbs_n == 0) return PZ_ERR_INVALID;
    size_t total = 0, a_in = 0, a_res = 0, a_eq = 0;
    PZCHK(pz_circuit_cells(kind, limbs_n, limb_bits, lookup_bits, n_steps_g, n_steps_r, &total, nullptr));
    PZCHK(pz_op_cells(0, limbs_n, limb_bits, lookup_bits, &a_in, nullptr));
    PZCHK(pz_op_cells(0, 2 * limbs_n, limb_bits, lookup_bits, &a_res, nullptr));
    PZCHK(pz_op_cells(5, 2 * limbs_n, limb_bits, lookup_bits, &a_eq, nullptr));
    if (total < 4 * a_in + a_res + a_eq) return PZ_ERR_INTERNAL;
    const size_t res = total - a_res - a_eq;
    cells.clear();
    if (kind == 3 || kind == 4) {
        // (kind 4, the weighted tally of n_steps_r + 1: ... | c_B | w_1 | .. | w_B | C, the weights' load_witness cells follow the
        // ciphertexts' blocks, one cell each)
        const size_t count = kind == 3 ? n_steps_g + 1 : n_steps_r + 1;
        for (uint32_t j = 0; j < limbs_n; ++j) cells.push_back(j);
        for (size_t i = 0; i < count; ++i)
            for (uint32_t j = 0; j < 2 * limbs_n; ++j) cells.push_back(a_in + i * a_res + j);
        if (kind == 4)
            for (size_t i = 0; i < count; ++i) cells.push_back(a_in + count * a_res + i);
        for (uint32_t j = 0; j < 2 * limbs_n; ++j) cells.push_back(res + j);
        return PZ_OK;
    }
    const unsigned heads = kind == 1 ? 4 : 2;   // n, g (, x = c1, y = c2)
    for (unsigned h = 0; h < heads; ++h)
        for (uint32_t j = 0; j < limbs_n; ++j) cells.push_back(h * a_in + j);
    if (kind == 5)   // "decrypt": n | g | m | c -- the message, the third assign_integer, moves into the statement; r stays private
        for (uint32_t j = 0; j < limbs_n; ++j) cells.push_back(2 * a_in + j);
    for (uint32_t j = 0; j < 2 * limbs_n; ++j) cells.push_back(res + j);
    return PZ_OK;
}

// the ballot (kind 6, `count` ciphertexts of m_bits-bit messages, n_steps_r records per r^n chain): n | g | c_1 | .. | c_K, then for
// K >= 2 the sum S.  n's and g's limb cells head the stream; the sum's last cell is the one in front of assign_integer(r_1); res_i is
// the assign_integer(2 limbs_n) in front of entry i's assert_equal_fresh, the K pairs closing the stream.
int ballot_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits, size_t n_steps_r,
                        std::vector<uint64_t>& cells) {
    if (limbs_n == 0) return PZ_ERR_INVALID;
    size_t total = 0, a_in = 0, a_res = 0, a_eq = 0;
    PZCHK(pz_ballot_cells(limbs_n, limb_bits, lookup_bits, count, m_bits, n_steps_r, &total, nullptr));
    PZCHK(pz_op_cells(0, limbs_n, limb_bits, lookup_bits, &a_in, nullptr));
    PZCHK(pz_op_cells(0, 2 * limbs_n, limb_bits, lookup_bits, &a_res, nullptr));
    PZCHK(pz_op_cells(5, 2 * limbs_n, limb_bits, lookup_bits, &a_eq, nullptr));
    if (total < 2 * a_in + count * (a_res + a_eq)) return PZ_ERR_INTERNAL;
    const size_t res = total - count * (a_res + a_eq);
    cells.clear();
    for (unsigned h = 0; h < 2; ++h)
        for (uint32_t j = 0; j < limbs_n; ++j) cells.push_back(h * a_in + j);
    for (size_t i = 0; i < count; ++i)
        for (uint32_t j = 0; j < 2 * limbs_n; ++j) cells.push_back(res + i * (a_res + a_eq) + j);
    if (count >= 2) cells.push_back(2 * a_in + count + 3 * (count - 1));
    return PZ_OK;
}

// a trustee's partial decryptions (kind 7, `count` ciphertexts): n | v | h | c_1 | u_1 | .. | c_K | u_K.  n's limb cells head the stream;
// v, theta and the c_j are the full-width assign_integer blocks that follow (theta is the witness: not exposed); h and the u_j are the
// assign_integer(2 limbs_n) in front of each of the count + 1 assert_equal_fresh closing the stream.
int partial_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, std::vector<uint64_t>& cells) {
    if (limbs_n == 0) return PZ_ERR_INVALID;
    size_t total = 0, a_in = 0, a_wide = 0, a_eq = 0;
    PZCHK(pz_partial_cells(limbs_n, limb_bits, lookup_bits, count, &total, nullptr));
    PZCHK(pz_op_cells(0, limbs_n, limb_bits, lookup_bits, &a_in, nullptr));
    PZCHK(pz_op_cells(0, 2 * limbs_n, limb_bits, lookup_bits, &a_wide, nullptr));
    PZCHK(pz_op_cells(5, 2 * limbs_n, limb_bits, lookup_bits, &a_eq, nullptr));
    if (total < a_in + (count + 2) * a_wide + (count + 1) * (a_wide + a_eq)) return PZ_ERR_INTERNAL;
    const size_t res = total - (count + 1) * (a_wide + a_eq);
    const uint32_t L = 2 * limbs_n;
    cells.clear();
    for (uint32_t j = 0; j < limbs_n; ++j) cells.push_back(j);
    for (uint32_t j = 0; j < L; ++j) cells.push_back(a_in + j);
    for (uint32_t j = 0; j < L; ++j) cells.push_back(res + j);
    for (size_t i = 1; i <= count; ++i) {
        for (uint32_t j = 0; j < L; ++j) cells.push_back(a_in + (1 + i) * a_wide + j);
        for (uint32_t j = 0; j < L; ++j) cells.push_back(res + i * (a_wide + a_eq) + j);
    }
    return PZ_OK;
}

// the mix (kind 8, `count` = 2^d ciphertexts, n_steps_r records per r^n chain): n | c_1 | .. | c_K | c'_1 | .. | c'_K.  n's limb cells head the
// stream, the c_j are the full-width assign_integer blocks that follow; c'_i is the assign_integer(2 limbs_n) in front of output i's
// assert_equal_fresh, the K pairs closing the stream.
int mix_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t n_steps_r, std::vector<uint64_t>& cells) {
    if (limbs_n == 0) return PZ_ERR_INVALID;
    size_t total = 0, a_in = 0, a_wide = 0, a_eq = 0;
    PZCHK(pz_mix_cells(limbs_n, limb_bits, lookup_bits, count, n_steps_r, &total, nullptr));
    PZCHK(pz_op_cells(0, limbs_n, limb_bits, lookup_bits, &a_in, nullptr));
    PZCHK(pz_op_cells(0, 2 * limbs_n, limb_bits, lookup_bits, &a_wide, nullptr));
    PZCHK(pz_op_cells(5, 2 * limbs_n, limb_bits, lookup_bits, &a_eq, nullptr));
    if (total < a_in + count * a_wide + count * (a_wide + a_eq)) return PZ_ERR_INTERNAL;
    const size_t res = total - count * (a_wide + a_eq);
    const uint32_t L = 2 * limbs_n;
    cells.clear();
    for (uint32_t j = 0; j < limbs_n; ++j) cells.push_back(j);
    for (size_t i = 0; i < count; ++i)
        for (uint32_t j = 0; j < L; ++j) cells.push_back(a_in + i * a_wide + j);
    for (size_t i = 0; i < count; ++i)
        for (uint32_t j = 0; j < L; ++j) cells.push_back(res + i * (a_wide + a_eq) + j);
    return PZ_OK;
}

// the short-randomness ballot (kind 9, `count` ciphertexts of m_bits-bit messages, exponents of s_limbs limbs): n | g | hs | c_1 | .. |
// c_K, then for K >= 2 the sum S.  n's and g's limb cells head the stream, hs is the full-width assign_integer that follows; the sum's
// last cell is the one in front of assign_integer(s_1); res_i is the assign_integer(2 limbs_n) in front of entry i's
// assert_equal_fresh, the K pairs closing the stream.
int sballot_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits, uint32_t s_limbs,
                         std::vector<uint64_t>& cells) {
    if (limbs_n == 0) return PZ_ERR_INVALID;
    size_t total = 0, a_in = 0, a_wide = 0, a_eq = 0;
    PZCHK(pz_sballot_cells(limbs_n, limb_bits, lookup_bits, count, m_bits, s_limbs, &total, nullptr));
    PZCHK(pz_op_cells(0, limbs_n, limb_bits, lookup_bits, &a_in, nullptr));
    PZCHK(pz_op_cells(0, 2 * limbs_n, limb_bits, lookup_bits, &a_wide, nullptr));
    PZCHK(pz_op_cells(5, 2 * limbs_n, limb_bits, lookup_bits, &a_eq, nullptr));
    if (total < 2 * a_in + a_wide + count * (a_wide + a_eq)) return PZ_ERR_INTERNAL;
    const size_t res = total - count * (a_wide + a_eq);
    const uint32_t L = 2 * limbs_n;
    cells.clear();
    for (unsigned h = 0; h < 2; ++h)
        for (uint32_t j = 0; j < limbs_n; ++j) cells.push_back(h * a_in + j);
    for (uint32_t j = 0; j < L; ++j) cells.push_back(2 * a_in + j);
    for (size_t i = 0; i < count; ++i)
        for (uint32_t j = 0; j < L; ++j) cells.push_back(res + i * (a_wide + a_eq) + j);
    if (count >= 2) cells.push_back(2 * a_in + a_wide + count + 3 * (count - 1));
    return PZ_OK;
}

// the short-randomness mix (kind 10, `count` = 2^d ciphertexts, exponents of s_limbs limbs): n | hs | c_1 | .. | c_K | c'_1 | .. | c'_K.
// n's limb cells head the stream, hs and the c_j are the 1 + K full-width assign_integer blocks that follow; c'_i is the
// assign_integer(2 limbs_n) in front of output i's assert_equal_fresh, the K pairs closing the stream.
int smix_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t s_limbs, std::vector<uint64_t>& cells) {
    if (limbs_n == 0) return PZ_ERR_INVALID;
    size_t total = 0, a_in = 0, a_wide = 0, a_eq = 0;
    PZCHK(pz_smix_cells(limbs_n, limb_bits, lookup_bits, count, s_limbs, &total, nullptr));
    PZCHK(pz_op_cells(0, limbs_n, limb_bits, lookup_bits, &a_in, nullptr));
    PZCHK(pz_op_cells(0, 2 * limbs_n, limb_bits, lookup_bits, &a_wide, nullptr));
    PZCHK(pz_op_cells(5, 2 * limbs_n, limb_bits, lookup_bits, &a_eq, nullptr));
    if (total < a_in + (count + 1) * a_wide + count * (a_wide + a_eq)) return PZ_ERR_INTERNAL;
    const size_t res = total - count * (a_wide + a_eq);
    const uint32_t L = 2 * limbs_n;
    cells.clear();
    for (uint32_t j = 0; j < limbs_n; ++j) cells.push_back(j);
    for (size_t i = 0; i <= count; ++i)
        for (uint32_t j = 0; j < L; ++j) cells.push_back(a_in + i * a_wide + j);
    for (size_t i = 0; i < count; ++i)
        for (uint32_t j = 0; j < L; ++j) cells.push_back(res + i * (a_wide + a_eq) + j);
    return PZ_OK;
}

// the packed ballot (kind 11, `count` ciphertexts of `slots` values of m_bits bits, exponents of s_limbs limbs): n | hs | G_0 | .. |
// G_{K-1} | c_1 | .. | c_R, then for K >= 2 the sums S_1 .. S_R.  n's limb cells head the stream, hs and the G_j are the 1 + K full-width
// assign_integer blocks that follow; behind them stand the R K load_witness cells and the R sums of 1 + 3 (K - 1) cells, the last cell of
// each its S_i; res_i is the assign_integer(2 limbs_n) in front of ciphertext i's assert_equal_fresh, the R pairs closing the stream.
int pballot_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t slots, uint32_t m_bits,
                         uint32_t s_limbs, std::vector<uint64_t>& cells) {
    if (limbs_n == 0) return PZ_ERR_INVALID;
    size_t total = 0, a_in = 0, a_wide = 0, a_eq = 0;
    PZCHK(pz_pballot_cells(limbs_n, limb_bits, lookup_bits, count, slots, m_bits, s_limbs, &total, nullptr));
    PZCHK(pz_op_cells(0, limbs_n, limb_bits, lookup_bits, &a_in, nullptr));
    PZCHK(pz_op_cells(0, 2 * limbs_n, limb_bits, lookup_bits, &a_wide, nullptr));
    PZCHK(pz_op_cells(5, 2 * limbs_n, limb_bits, lookup_bits, &a_eq, nullptr));
    if (total < a_in + (slots + 1) * a_wide + count * (a_wide + a_eq)) return PZ_ERR_INTERNAL;
    const size_t res = total - count * (a_wide + a_eq), K = slots;
    const uint32_t L = 2 * limbs_n;
    cells.clear();
    for (uint32_t j = 0; j < limbs_n; ++j) cells.push_back(j);
    for (size_t i = 0; i <= K; ++i)
        for (uint32_t j = 0; j < L; ++j) cells.push_back(a_in + i * a_wide + j);
    for (size_t i = 0; i < count; ++i)
        for (uint32_t j = 0; j < L; ++j) cells.push_back(res + i * (a_wide + a_eq) + j);
    if (K >= 2) {
        const size_t sums = a_in + (K + 1) * a_wide + count * K, per_sum = 1 + 3 * (K - 1);
        for (size_t i = 0; i < count; ++i) cells.push_back(sums + (i + 1) * per_sum - 1);
    }
    return PZ_OK;
}

}   // namespace

int pz_instance_eval_launch(pz_ctx* ctx, uint32_t k, const uint64_t omega[4], const uint64_t n_inv[4], const uint64_t* d_instances, size_t L,
                            size_t B, const uint64_t* d_x, size_t x_stride, uint64_t* d_out, size_t out_stride, int32_t* d_flags) {
    if (!B) return PZ_OK;
    const size_t chunks = (L + IT * IE - 1) / (IT * IE);
    if (chunks > 0x7fffffffu) return PZ_ERR_UNSUPPORTED;
    void* partial = nullptr;
    PZCHK(pz_ws_get(ctx, WS_MISC, B * (chunks ? chunks : 1) * 32, &partial));
    HIPCHK(ctx, hipMemsetAsync(d_flags, 0, B * 4, ctx->stream));
    for (size_t b0 = 0; b0 < B && chunks; b0 += 65535) {   // (the grid's second dimension holds 65535 proofs)
        const size_t nb = B - b0 < 65535 ? B - b0 : 65535;
        hipLaunchKernelGGL(k_instance_eval, dim3((unsigned)chunks, (unsigned)nb), dim3(IT), 0, ctx->stream, d_instances + b0 * L * 4, L,
                           d_x + b0 * x_stride, x_stride, w4_of(omega), (uint64_t*)partial + b0 * chunks * 4, d_flags + b0);
        HIPCHK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_instance_finish, dim3(pz_div_up(B, 64)), dim3(64), 0, ctx->stream, (const uint64_t*)partial, (unsigned)chunks, B, d_x, x_stride,
                       k, w4_of(n_inv), d_out, out_stride, d_flags);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_instance_eval_dev(pz_ctx* ctx, uint32_t k, const uint64_t omega[4], const uint64_t n_inv[4], const uint64_t* d_instances,
                                    size_t n_public, size_t n_proofs, const uint64_t* d_x, uint64_t* d_out, int32_t* d_flags) {
    if (!ctx || !omega || !n_inv || !d_x || !d_out || !d_flags || (n_public && !d_instances)) return PZ_ERR_INVALID;
    if (k < 1 || k > 28 || n_public > ((size_t)1 << k)) return PZ_ERR_INVALID;
    PZ_ENTER(ctx);
    return pz_instance_eval_launch(ctx, k, omega, n_inv, d_instances, n_public, n_proofs, d_x, 4, d_out, 4, d_flags);
}

// the statement's cells of any kind, an allocation failure as a status.  count (and m_bits) are the ballots', the partial decryption's
// and the mix's; n_steps_g is the by-kind circuits'
static int statement_cells(int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits, size_t n_steps_g,
                           size_t n_steps_r, std::vector<uint64_t>& cells, uint32_t slots = 0) {
    try {
        if (kind == 6) return ballot_public_cells(limbs_n, limb_bits, lookup_bits, count, m_bits, n_steps_r, cells);
        if (kind == 7) return partial_public_cells(limbs_n, limb_bits, lookup_bits, count, cells);
        if (kind == 8) return mix_public_cells(limbs_n, limb_bits, lookup_bits, count, n_steps_r, cells);
        if (kind == 9)   // (n_steps_r: the 2 s_limbs limb_bits records of one hs-chain)
            return sballot_public_cells(limbs_n, limb_bits, lookup_bits, count, m_bits, (uint32_t)(n_steps_r / (2 * (size_t)limb_bits)), cells);
        if (kind == 10) return smix_public_cells(limbs_n, limb_bits, lookup_bits, count, (uint32_t)(n_steps_r / (2 * (size_t)limb_bits)), cells);
        if (kind == 11)
            return pballot_public_cells(limbs_n, limb_bits, lookup_bits, count, slots, m_bits, (uint32_t)(n_steps_r / (2 * (size_t)limb_bits)),
                                        cells);
        return public_cells(kind, limbs_n, limb_bits, lookup_bits, n_steps_g, n_steps_r, cells);
    } catch (const std::bad_alloc&) {
        return PZ_ERR_OOM;
    }
}
// the tail of the seven pz_*_public_cells entry points: the count always, the cells where the caller gave room
static int public_cells_out(int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits, size_t n_steps_g,
                            size_t n_steps_r, uint64_t* cells_out, size_t capacity, size_t* n_public, uint32_t slots = 0) {
    if (!n_public) return PZ_ERR_INVALID;
    std::vector<uint64_t> cells;
    PZCHK(statement_cells(kind, limbs_n, limb_bits, lookup_bits, count, m_bits, n_steps_g, n_steps_r, cells, slots));
    *n_public = cells.size();
    if (cells_out) {
        if (capacity < cells.size()) return PZ_ERR_CAPACITY;
        memcpy(cells_out, cells.data(), cells.size() * 8);
    }
    return PZ_OK;
}

extern "C" int pz_circuit_public_cells(int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t n_steps_g, size_t n_steps_r,
                                       uint64_t* cells_out, size_t capacity, size_t* n_public) {
    if (kind > 5) return PZ_ERR_INVALID;   // (kinds 6 to 11 have entry points of their own)
    return public_cells_out(kind, limbs_n, limb_bits, lookup_bits, 0, 0, n_steps_g, n_steps_r, cells_out, capacity, n_public);
}
extern "C" int pz_ballot_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits, size_t n_steps_r,
                                      uint64_t* cells_out, size_t capacity, size_t* n_public) {
    return public_cells_out(6, limbs_n, limb_bits, lookup_bits, count, m_bits, 0, n_steps_r, cells_out, capacity, n_public);
}
extern "C" int pz_partial_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint64_t* cells_out,
                                       size_t capacity, size_t* n_public) {
    return public_cells_out(7, limbs_n, limb_bits, lookup_bits, count, 0, 0, 0, cells_out, capacity, n_public);
}
extern "C" int pz_mix_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t n_steps_r,
                                   uint64_t* cells_out, size_t capacity, size_t* n_public) {
    return public_cells_out(8, limbs_n, limb_bits, lookup_bits, count, 0, 0, n_steps_r, cells_out, capacity, n_public);
}

extern "C" int pz_sballot_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits,
                                       uint32_t s_limbs, uint64_t* cells_out, size_t capacity, size_t* n_public) {
    if (limb_bits == 0) return PZ_ERR_INVALID;
    return public_cells_out(9, limbs_n, limb_bits, lookup_bits, count, m_bits, 0, 2 * (size_t)s_limbs * limb_bits, cells_out, capacity, n_public);
}

extern "C" int pz_smix_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t s_limbs,
                                    uint64_t* cells_out, size_t capacity, size_t* n_public) {
    if (limb_bits == 0) return PZ_ERR_INVALID;
    return public_cells_out(10, limbs_n, limb_bits, lookup_bits, count, 0, 0, 2 * (size_t)s_limbs * limb_bits, cells_out, capacity, n_public);
}

extern "C" int pz_pballot_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t slots, uint32_t m_bits,
                                       uint32_t s_limbs, uint64_t* cells_out, size_t capacity, size_t* n_public) {
    if (limb_bits == 0) return PZ_ERR_INVALID;
    return public_cells_out(11, limbs_n, limb_bits, lookup_bits, count, m_bits, 0, 2 * (size_t)s_limbs * limb_bits, cells_out, capacity, n_public,
                            slots);
}

extern "C" int pz_structure_expose(pz_structure* st) {
    if (!st || !st->ctx || st->n_instance) return PZ_ERR_INVALID;
    pz_ctx* ctx = st->ctx;
    PZ_ENTER(ctx);
    std::vector<uint64_t> cells;
    PZCHK(statement_cells(st->kind, st->limbs_n, st->limb_bits, st->lookup_bits, st->count, (uint32_t)(st->n_steps_g / 2), st->n_steps_g,
                          st->n_steps_r, cells, st->slots));   // (the ballots' m_bits: their g-chains take 2 m_bits records)
    const size_t L = cells.size(), m = st->n_adv + st->n_lk + 1, n = (size_t)1 << st->k;
    if (L > st->max_rows) return PZ_ERR_UNSUPPORTED;   // (a tally of many ciphertexts: the statement must fit the column's usable rows)
    if (L == 0 || cells.back() >= st->n_cells) return PZ_ERR_INTERNAL;
    if (m + 1 > ((size_t)1 << 32) / n) return PZ_ERR_UNSUPPORTED;   // the copy-constraint map addresses cells with 32 bits
    // device buffers of this call (released on every path out) and the structure's new arrays (handed over at the end)
    struct Bufs {
        std::vector<void*> v;
        ~Bufs() {
            for (void* d : v)
                if (d) (void)pz_hip_free(d);
        }
        int get(pz_ctx* c, size_t bytes, void** out) {
            HIPCHK(c, pz_hip_malloc(c, out, bytes ? bytes : 1));
            v.push_back(*out);
            return PZ_OK;
        }
    } tmp;
    void *d_cells, *d_e, *d_f, *d_err, *d_link, *cc, *cr, *mc, *mr;
    PZCHK(tmp.get(ctx, L * 8, &d_cells)); PZCHK(tmp.get(ctx, L * 8, &d_e)); PZCHK(tmp.get(ctx, L * 8, &d_f)); PZCHK(tmp.get(ctx, 4, &d_err));
    PZCHK(tmp.get(ctx, L * 8, &d_link));
    PZCHK(tmp.get(ctx, L * 4, &cc)); PZCHK(tmp.get(ctx, L * 4, &cr));
    PZCHK(tmp.get(ctx, (m + 1) * n * 4, &mc)); PZCHK(tmp.get(ctx, (m + 1) * n * 4, &mr));
    HIPCHK(ctx, hipMemcpyAsync(d_cells, cells.data(), L * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_err, 0, 4, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(mc, st->d_map_col, m * n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(mr, st->d_map_row, m * n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_public_pos, dim3(pz_div_up(L, 64)), dim3(64), 0, ctx->stream, (const uint64_t*)d_cells, L, (const uint64_t*)st->d_starts,
                       (int)st->n_used, (uint32_t*)cc, (uint32_t*)cr);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_public_find, dim3(pz_div_up(L, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)st->d_map_col, (const uint32_t*)st->d_map_row,
                       (uint64_t)n, (uint64_t)(m * n), (const uint32_t*)cc, (const uint32_t*)cr, L, (uint64_t*)d_e, (uint64_t*)d_f, (unsigned*)d_err);
    HIPCHK(ctx, hipGetLastError());
    // the classes' last cells come back once: grouping the exposed rows by class is a sort of L keys, done on the host
    unsigned err = 0;
    std::vector<uint32_t> link;
    try {
        std::vector<uint64_t> e(L);
        HIPCHK(ctx, hipMemcpyAsync(e.data(), d_e, L * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (err) return PZ_ERR_INTERNAL;
        class_links(e, link);
    } catch (const std::bad_alloc&) {
        return PZ_ERR_OOM;
    }
    HIPCHK(ctx, hipMemcpyAsync(d_link, link.data(), L * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_public_link, dim3(pz_div_up(n, 256)), dim3(256), 0, ctx->stream, (uint32_t*)mc, (uint32_t*)mr, (uint64_t)n, (uint32_t)m, L,
                       (const uint64_t*)d_e, (const uint64_t*)d_f, (const uint32_t*)d_link);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // the (m + 1)-column maps replace the structure's (the old ones are released with this call's scratch); the cell positions stay
    for (void*& d : tmp.v) {
        if (d == mc) d = st->d_map_col;
        else if (d == mr) d = st->d_map_row;
        else if (d == cc || d == cr) d = nullptr;
    }
    st->d_map_col = (uint32_t*)mc;
    st->d_map_row = (uint32_t*)mr;
    st->d_cell_col = (uint32_t*)cc;
    st->d_cell_row = (uint32_t*)cr;
    st->n_instance = 1;
    st->n_public = L;
    return PZ_OK;
}

extern "C" int pz_structure_public(const pz_structure* st, size_t* n_instance, size_t* n_public, const uint32_t** d_cell_col,
                                   const uint32_t** d_cell_row) {
    if (!st) return PZ_ERR_INVALID;
    if (n_instance) *n_instance = st->n_instance;
    if (n_public) *n_public = st->n_public;
    if (d_cell_col) *d_cell_col = st->d_cell_col;
    if (d_cell_row) *d_cell_row = st->d_cell_row;
    return PZ_OK;
}

extern "C" int pz_public_gather_dev(pz_ctx* ctx, const uint64_t* d_cols, size_t col_stride, const uint32_t* d_cell_col, const uint32_t* d_cell_row,
                                    size_t n_public, uint64_t* out_words) {
    if (!ctx || !d_cols || !d_cell_col || !d_cell_row || !out_words || !n_public || col_stride < 4) return PZ_ERR_INVALID;
    if (col_stride % 4 || ((uintptr_t)d_cols & 15)) return PZ_ERR_INVALID;   // elements are read as two 16-byte words
    PZ_ENTER(ctx);
    void* d_out = nullptr;
    PZCHK(pz_ws_get(ctx, WS_MISC, n_public * 32, &d_out));
    hipLaunchKernelGGL(k_public_gather, dim3(pz_div_up(n_public, 64)), dim3(64), 0, ctx->stream, d_cols, col_stride, d_cell_col, d_cell_row, n_public,
                       (uint64_t*)d_out);
    HIPCHK(ctx, hipGetLastError());
    return pz_download(ctx, out_words, d_out, n_public * 32);
}
