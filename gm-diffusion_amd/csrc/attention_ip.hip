// Decoupled cross-attention of an IP-Adapter (diffusers' IPAdapterAttnProcessor) as ONE launch:
//   O = softmax(s Q K_text^T) V_text  +  ip_scale * softmax(s Q K_ip^T) V_ip
// Two launches of gmd_attention and an add read Q twice and write O, read it back and write it again; here Q is read once
// and O stored once, and nothing in between reaches global memory.
//
// The transposed formulation of attention.hip (S^T = K Q^T, O^T += V^T P^T: the softmax state of a query lives on one lane, the
// score accumulator becomes the B operand of the second product in place), one workgroup = 4 waves = 128 queries of one
// (batch, head), K / V^T tiles of 64 keys staged through registers into two LDS stages.  Order of work:
//   1. the text keys, tile after tile, with the classic (maximum-first) online softmax: running maximum m and row sum l;
//   2. the accumulator is normalised in place: ot *= 1 / l_text;
//   3. the image keys -- at most 64, ONE tile, prefetched as "the tile after the last text tile" -- with a maximum and a row
//      sum OF THEIR OWN (a softmax over few keys must not inherit the stabiliser or the normaliser of the other: with a shared
//      maximum the weaker branch underflows to zero, with a shared row sum the two are one softmax over 77 + Nip keys);
//   4. ot += (ip_scale / l_ip) * (V_ip^T P_ip^T), one 32-row tile of O^T at a time (16 temporary registers, not a second
//      accumulator set), in float32;
//   5. one rounding to the 16-bit type, row-contiguous store through LDS as in attention.hip.
// Both row sums are taken from the unrounded float32 probabilities on the vector ALU (the matrix-core row sum of attention.hip
// needs a spare V^T row, which head dims 32, 64 and 160 do not have; with two key tiles it buys nothing).  Q is not rescaled:
// the softmax scale multiplies the float32 scores.
// ip_scale is read from DEVICE memory, so one captured graph serves every scale (the ControlNet precedent, controlnet.hip).
#include "gmd_common.h"

#include <type_traits>

namespace {

struct AttnIpParams {
    const bf16_t* Q;
    const bf16_t* K;
    const bf16_t* Vt;
    const bf16_t* Kip;
    const bf16_t* Vtip;
    bf16_t* O;
    const float* ip_scale;  // the entry this launch reads (array base + index)
    int Nq, Nk, Nip, H;
    int64_t ldq, ldk, ldvt, ldkip, ldvtip, ldo, sQ, sK, sVt, sKip, sVtip, sO;
    float scale_log2;  // softmax scale * log2(e)
};

constexpr int KV = 64;     // keys per tile
constexpr int VROW = 136;  // bytes per V^T LDS row: 64 keys * 2 B + 8 B pad (conflict-free b64 reads)
constexpr float kNegBig = -1.0e30f;

template <typename HT, int D>
__global__ __launch_bounds__(256, D <= 64 ? 2 : 1) void attn_ip_kernel(const AttnIpParams p) {
    GMD_WG_TRACE_SCOPE(WGK_ATTN);
    constexpr int DK = (D + 15) / 16;        // 16-wide k-steps of Q K^T over d
    constexpr int DT = (D + 31) / 32;        // 32-row tiles of O^T over d
    constexpr int KROW = (2 * DK + 1) * 16;  // bytes per K LDS row: odd number of 16-byte slots
    constexpr int DC = D / 8;                // 16-byte chunks per K row in global memory
    static_assert(D % 8 == 0, "head dim must be a multiple of 8");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int kStageBytes = KV * KROW + DT * 32 * VROW;  // K tile [KV][KROW] + V^T tile [DT*32][VROW]
    constexpr int NKC = (KV * DC + 255) / 256;               // 16-byte K chunks staged per thread
    constexpr int NVC = (D * 8 + 255) / 256;                 // 16-byte V^T chunks staged per thread

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    // XCD-aware order of the workgroups, as in attention.hip: the query blocks of one (batch, head) share one L2
    int qb, head, b;
    {
        const int nwg = gridDim.x, id = blockIdx.x;
        const int qq = nwg >> 3, rr = nwg & 7, xcd = id & 7, j = id >> 3;
        const int L = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + j;
        const int nqb = (p.Nq + 127) / 128;
        qb = L % nqb;
        const int t = L / nqb;
        head = t % p.H;
        b = t / p.H;
    }
    const int q = qb * 128 + wid * 32 + r;
    const bool qvalid = q < p.Nq;
    const bf16_t* Qb = p.Q + (int64_t)b * p.sQ + (int64_t)head * D;

    // zero the LDS padding that is read but never staged (both stages): K columns [D, DK*16), V^T rows [D, DT*32)
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        unsigned char* Ks0 = smem + st * kStageBytes;
        unsigned char* Vs0 = Ks0 + KV * KROW;
        if (DK * 16 > D) {
            for (int i = tid; i < KV; i += 256) *reinterpret_cast<uint4*>(Ks0 + i * KROW + DC * 16) = make_uint4(0, 0, 0, 0);
        }
        for (int i = tid; i < (DT * 32 - D) * (VROW / 8); i += 256) {
            const int row = D + i / (VROW / 8), c = i % (VROW / 8);
            *reinterpret_cast<uint2*>(Vs0 + row * VROW + c * 8) = make_uint2(0, 0);
        }
    }

    // Q fragments (B operand of the first product), loaded ONCE for both branches: lane (r, hh) element j = Q[q][16 s + 8 hh + j]
    uint4 qf[DK];
#pragma unroll
    for (int s = 0; s < DK; ++s) {
        const int d0 = 16 * s + 8 * hh;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (qvalid && d0 + 8 <= D) v = *reinterpret_cast<const uint4*>(Qb + (int64_t)q * p.ldq + d0);
        qf[s] = v;
    }

    f32x16 ot[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) ot[t][i] = 0.f;

    // Register staging of the next tile (issued before the MFMAs of the current one, written to the other LDS stage after them).
    // Raw buffer loads: rows of K at or beyond the key count and the slots a thread does not own fall outside the descriptor's
    // range and read as zeros.  The two key sets differ in base, leading dimensions and count only.
    uint4 kreg[NKC], vreg[NVC];
    auto as_u4 = [](auto v) { return *reinterpret_cast<uint4*>(&v); };
    auto load_kv = [&](const bf16_t* Kb, const bf16_t* Vb, int ldk, int ldvt, int n, int k0) {
        const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)Kb, 0, (int)((((int64_t)n - 1) * ldk + D) * 2), 0x00020000);
        const __amdgpu_buffer_rsrc_t rsV =
            __builtin_amdgcn_make_buffer_rsrc((void*)Vb, 0, (int)((((int64_t)D - 1) * ldvt + (n + 7) / 8 * 8) * 2), 0x00020000);
        // the tile offset is part of the per-lane offset, which is what the range check sees (a scalar offset is not checked)
        const unsigned ksoff = (unsigned)(k0 * ldk * 2), vsoff = (unsigned)(k0 * 2);
#pragma unroll
        for (int u = 0; u < NKC; ++u) {
            const int id = tid + 256 * u, key = id / DC;
            const unsigned ofs = id < KV * DC ? (unsigned)((key * ldk + (id - key * DC) * 8) * 2) : 0x7fffffffu;
            kreg[u] = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rsK, (int)(ofs + ksoff), 0, 0));
        }
#pragma unroll
        for (int u = 0; u < NVC; ++u) {
            const int id = tid + 256 * u;
            const unsigned ofs = id < D * 8 ? (unsigned)(((id >> 3) * ldvt + (id & 7) * 8) * 2) : 0x7fffffffu;
            vreg[u] = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rsV, (int)(ofs + vsoff), 0, 0));
        }
        if (k0 + KV <= n) return;  // full tile (wave-uniform)
        // partial tile: V^T columns of keys >= n (row padding, or the next row's keys) are staged as zeros; their scores are
        // masked as well
#pragma unroll
        for (int u = 0; u < NVC; ++u) {
            const int nv = n - (k0 + ((tid + 256 * u) & 7) * 8);  // valid elements in this chunk
            if (nv < 8) {
                unsigned w[4] = {vreg[u].x, vreg[u].y, vreg[u].z, vreg[u].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (2 * e >= nv) w[e] = 0;
                    else if (2 * e + 1 >= nv) w[e] &= 0xffffu;
                }
                vreg[u] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    };
    auto store_kv = [&](int st) {
        unsigned char* Ks0 = smem + st * kStageBytes;
        unsigned char* Vs0 = Ks0 + KV * KROW;
#pragma unroll
        for (int u = 0; u < NKC; ++u) {
            const int id = tid + 256 * u;
            const int key = id / DC, ch = id - key * DC;
            if (id < KV * DC) *reinterpret_cast<uint4*>(Ks0 + key * KROW + ch * 16) = kreg[u];
        }
#pragma unroll
        for (int u = 0; u < NVC; ++u) {
            const int id = tid + 256 * u;
            const int d = id >> 3, ch = id & 7;
            if (id < D * 8) {
                unsigned char* dst = Vs0 + d * VROW + ch * 16;
                *reinterpret_cast<uint2*>(dst) = make_uint2(vreg[u].x, vreg[u].y);
                *reinterpret_cast<uint2*>(dst + 8) = make_uint2(vreg[u].z, vreg[u].w);
            }
        }
    };
    const bf16_t* Kb = p.K + (int64_t)b * p.sK + (int64_t)head * D;
    const bf16_t* Vb = p.Vt + (int64_t)b * p.sVt + (int64_t)head * D * p.ldvt;
    const bf16_t* Kipb = p.Kip + (int64_t)b * p.sKip + (int64_t)head * D;
    const bf16_t* Vipb = p.Vtip + (int64_t)b * p.sVtip + (int64_t)head * D * p.ldvtip;
    auto load_text = [&](int k0) { load_kv(Kb, Vb, (int)p.ldk, (int)p.ldvt, p.Nk, k0); };
    auto load_image = [&]() { load_kv(Kipb, Vipb, (int)p.ldkip, (int)p.ldvtip, p.Nip, 0); };

    const float c = p.scale_log2;

    // S^T = K Q^T of the 64-key tile in stage Ks whose first key is k0 of n; keys at and beyond n masked.  The second 32-key
    // half is not multiplied when it holds no key (wave-uniform).
    auto scores = [&](const unsigned char* Ks, int k0, int n, f32x16 (&st)[2]) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int i = 0; i < 16; ++i) st[t][i] = 0.f;
            if (t == 0 || k0 + 32 < n) {
#pragma unroll
                for (int s = 0; s < DK; ++s) {
                    const uint4 kf = *reinterpret_cast<const uint4*>(Ks + (32 * t + r) * KROW + (2 * s + hh) * 16);
                    st[t] = Half<HT>::mfma32(kf, qf[s], st[t]);
                }
            }
        }
        if (k0 + KV > n) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = k0 + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * hh;
                    if (key >= n) st[t][i] = kNegBig;
                }
        }
    };
    // One step of the online softmax on a score tile: st becomes P = 2^((s - m) c); m_run / l_run are the state of ONE branch
    // (query = lane & 31; this half-wave holds 32 of the 64 keys, l_run is its partial row sum).  Returns the factor by which
    // what was accumulated against the old maximum shrinks.
    auto softmax_tile = [&](f32x16 (&st)[2], float& m_run, float& l_run) {
        float mx = fmaxf(st[0][0], st[1][0]);
#pragma unroll
        for (int i = 1; i < 16; ++i) mx = fmaxf(fmaxf(mx, st[0][i]), st[1][i]);
        mx = half_swap_max(mx);
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
        const float mc = m_new * c;
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float pv = __builtin_amdgcn_exp2f(st[t][i] * c - mc);
                st[t][i] = pv;
                psum += pv;
            }
        l_run = l_run * alpha + psum;
        return alpha;
    };
    // P^T -> 16-bit B fragments: k-step ks = 2 t + s uses registers 8 s .. 8 s + 7 of tile t
    auto pack_p = [&](const f32x16 (&st)[2], uint4 (&pf)[4]) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                uint4 w;
                w.x = Half<HT>::pack2(st[t][8 * s + 0], st[t][8 * s + 1]);
                w.y = Half<HT>::pack2(st[t][8 * s + 2], st[t][8 * s + 3]);
                w.z = Half<HT>::pack2(st[t][8 * s + 4], st[t][8 * s + 5]);
                w.w = Half<HT>::pack2(st[t][8 * s + 6], st[t][8 * s + 7]);
                pf[2 * t + s] = w;
            }
    };
    // acc += V^T P^T for the 32 rows dt of O^T; nloc = keys of this tile that exist (a k-step covers 16 of them)
    auto second_product = [&](const unsigned char* Vs, const uint4 (&pf)[4], int dt, int nloc, f32x16 acc) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (16 * ks < nloc) {
                // element j of lane half hh is key 16 ks + 8 (j>>2) + 4 hh + (j&3) of this 64-key tile
                const unsigned char* src = Vs + (32 * dt + r) * VROW + (16 * ks + 4 * hh) * 2;
                const uint2 lo = *reinterpret_cast<const uint2*>(src);
                const uint2 hi = *reinterpret_cast<const uint2*>(src + 16);
                acc = Half<HT>::mfma32(make_uint4(lo.x, lo.y, hi.x, hi.y), pf[ks], acc);
            }
        }
        return acc;
    };

    // ---- 1. text keys ----
    const int ntiles = (p.Nk + KV - 1) / KV;
    float m_text = kNegBig, l_text = 0.f;
    auto text_tile = [&](const int kt, auto stage_c) {
        const int STAGE = stage_c;
        const int k0 = kt * KV;
        const unsigned char* Ks = smem + STAGE * kStageBytes;
        const unsigned char* Vs = Ks + KV * KROW;
        // prefetch into registers: the next text tile, or behind the last one the image tile
        if (kt + 1 < ntiles) load_text(k0 + KV);
        else load_image();
        f32x16 st[2];
        scores(Ks, k0, p.Nk, st);
        const float alpha = softmax_tile(st, m_text, l_text);
        if (!__all(alpha == 1.0f)) {  // wave-uniform: no running maximum of this wave moved -> no rescale
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) ot[t][i] *= alpha;
        }
        uint4 pf[4];
        pack_p(st, pf);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) ot[dt] = second_product(Vs, pf, dt, p.Nk - k0, ot[dt]);
        store_kv(STAGE ^ 1);  // that stage was last read in iteration kt-1
        __syncthreads();
    };
    load_text(0);
    __syncthreads();  // padding fill visible before the first stage is written around it
    store_kv(0);
    __syncthreads();
    for (int kt = 0; kt < ntiles; kt += 2) {
        text_tile(kt, std::integral_constant<int, 0>{});
        if (kt + 1 < ntiles) text_tile(kt + 1, std::integral_constant<int, 1>{});
    }

    // ---- 2. normalise the text branch in place ----
    {
        const float inv = 1.0f / half_swap_sum(l_text);
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) ot[t][i] *= inv;
    }

    // ---- 3. / 4. image keys: one tile, its own maximum and row sum ----
    {
        const unsigned char* Ks = smem + (ntiles & 1) * kStageBytes;
        const unsigned char* Vs = Ks + KV * KROW;
        f32x16 st[2];
        scores(Ks, 0, p.Nip, st);
        float m_ip = kNegBig, l_ip = 0.f;
        softmax_tile(st, m_ip, l_ip);
        const float f = *p.ip_scale / half_swap_sum(l_ip);
        uint4 pf[4];
        pack_p(st, pf);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            f32x16 oi;
#pragma unroll
            for (int i = 0; i < 16; ++i) oi[i] = 0.f;
            oi = second_product(Vs, pf, dt, p.Nip, oi);
#pragma unroll
            for (int i = 0; i < 16; ++i) ot[dt][i] += f * oi[i];
        }
    }
    __syncthreads();  // every wave is done reading the stages: they become the store strips

    // ---- 5. store: lane owns query q, registers hold d = 32 dt + 8 g + 4 hh + i; row-contiguous through LDS ----
    constexpr int SROW = D * 2 + 16;  // strip row stride in bytes (pad: spreads the rows over the banks)
    static_assert(4 * 32 * SROW <= 2 * kStageBytes, "the four strips fit the two stages");
    unsigned char* strip = smem + wid * (32 * SROW);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d0 = 32 * dt + 8 * g + 4 * hh;
            if (d0 < D) {
                uint2 w;
                w.x = Half<HT>::pack2(ot[dt][4 * g + 0], ot[dt][4 * g + 1]);
                w.y = Half<HT>::pack2(ot[dt][4 * g + 2], ot[dt][4 * g + 3]);
                *reinterpret_cast<uint2*>(strip + r * SROW + d0 * 2) = w;
            }
        }
    __builtin_amdgcn_wave_barrier();  // same wave, in-order LDS: a compiler fence only
    constexpr int CH = D / 8;         // 16-byte chunks per query row
    const int q0w = qb * 128 + wid * 32;
    bf16_t* Ow = p.O + (int64_t)b * p.sO + (int64_t)q0w * p.ldo + (int64_t)head * D;
#pragma unroll
    for (int t = 0; t < (32 * CH + 63) / 64; ++t) {
        const int idx = lane + 64 * t;
        const int rr = idx / CH, cc = idx - rr * CH;
        if (rr < 32 && q0w + rr < p.Nq)
            *reinterpret_cast<uint4*>(Ow + (int64_t)rr * p.ldo + cc * 8) = *reinterpret_cast<const uint4*>(strip + rr * SROW + cc * 16);
    }
}

template <typename HT, int D>
int launch_attn_ip(const AttnIpParams& p, int B, int H, hipStream_t s) {
    constexpr int DK = (D + 15) / 16, DT = (D + 31) / 32;
    const size_t smem = 2 * ((size_t)KV * (2 * DK + 1) * 16 + (size_t)DT * 32 * VROW);  // two stages
    dim3 grid(((p.Nq + 127) / 128) * H * B, 1, 1);                                      // 1-D: remapped per XCD in the kernel
    attn_ip_kernel<HT, D><<<grid, 256, smem, s>>>(p);
    GMD_CHECK_LAUNCH("gmd_attention_ip");
    return GMD_OK;
}

template <typename HT>
int dispatch_attn_ip(const AttnIpParams& p, int B, int H, int D, hipStream_t s) {
    switch (D) {
        case 32: return launch_attn_ip<HT, 32>(p, B, H, s);
        case 40: return launch_attn_ip<HT, 40>(p, B, H, s);
        case 64: return launch_attn_ip<HT, 64>(p, B, H, s);
        case 80: return launch_attn_ip<HT, 80>(p, B, H, s);
        case 160: return launch_attn_ip<HT, 160>(p, B, H, s);
        default:
            gmd_set_error("gmd_attention_ip: head dim %d not instantiated (supported: 32, 40, 64, 80, 160)", D);
            return GMD_ERR_UNSUPPORTED;
    }
}

}  // namespace

extern "C" int gmd_attention_ip(const void* Q, const void* K, const void* Vt, const void* Kip, const void* Vtip, void* O, int dtype, int B,
                                int H, int D, int Nq, int Nk, int Nip, int64_t ldq, int64_t ldk, int64_t ldvt, int64_t ldkip,
                                int64_t ldvtip, int64_t ldo, int64_t strideQ, int64_t strideK, int64_t strideVt, int64_t strideKip,
                                int64_t strideVtip, int64_t strideO, float softmax_scale, const float* ip_scale, int ip_scale_index,
                                gmd_stream_t stream) {
    if (dtype != GMD_BF16 && dtype != GMD_F16) {
        gmd_set_error("gmd_attention_ip: GMD_BF16 / GMD_F16 are implemented (float32 composes gmd_attention twice and gmd_scaled_add)");
        return GMD_ERR_UNSUPPORTED;
    }
    GMD_REQUIRE(B >= 0 && H > 0 && Nq >= 0 && Nk > 0, "gmd_attention_ip: bad shape B=%d H=%d Nq=%d Nk=%d", B, H, Nq, Nk);
    GMD_REQUIRE(Nip >= 1 && Nip <= KV, "gmd_attention_ip: Nip=%d outside [1, %d] (the image keys are one tile)", Nip, KV);
    GMD_REQUIRE(ip_scale != nullptr && ip_scale_index >= 0, "gmd_attention_ip: ip_scale must be a device array, the index non-negative");
    if (B == 0 || Nq == 0) return GMD_OK;  // empty batch / no queries: nothing to write
    GMD_REQUIRE((int64_t)((Nq + 127) / 128) * H * B < (1ll << 31), "gmd_attention_ip: grid too large");
    GMD_REQUIRE(Q && K && Vt && Kip && Vtip && O, "gmd_attention_ip: null pointer");
    GMD_REQUIRE(gmd_aligned16(Q) && gmd_aligned16(K) && gmd_aligned16(Vt) && gmd_aligned16(Kip) && gmd_aligned16(Vtip) && gmd_aligned16(O),
                "gmd_attention_ip: pointers must be 16-byte aligned");
    GMD_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldkip % 8 == 0 && ldvtip % 8 == 0 && ldo % 8 == 0,
                "gmd_attention_ip: leading dimensions must be multiples of 8");
    GMD_REQUIRE(strideQ % 8 == 0 && strideK % 8 == 0 && strideVt % 8 == 0 && strideKip % 8 == 0 && strideVtip % 8 == 0 && strideO % 8 == 0,
                "gmd_attention_ip: batch strides must be multiples of 8");
    // the staging addresses a whole 64-key tile with 32-bit byte offsets, also where the last tile is partial
    const int64_t nk_tiles = ((int64_t)Nk + KV - 1) / KV * KV;
    GMD_REQUIRE(nk_tiles * ldk < (1ll << 30) && (int64_t)D * ldvt < (1ll << 30) && (int64_t)KV * ldkip < (1ll << 30) &&
                    (int64_t)D * ldvtip < (1ll << 30),
                "gmd_attention_ip: K / V^T slab of one head exceeds 2 GiB");
    GMD_REQUIRE(ldvt >= ((Nk + 7) / 8) * 8, "gmd_attention_ip: ldvt=%lld must cover Nk=%d rounded up to 8", (long long)ldvt, Nk);
    GMD_REQUIRE(ldvtip >= ((Nip + 7) / 8) * 8, "gmd_attention_ip: ldvtip=%lld must cover Nip=%d rounded up to 8", (long long)ldvtip, Nip);
    GMD_REQUIRE(ldq >= (int64_t)H * D && ldk >= (int64_t)H * D && ldkip >= (int64_t)H * D && ldo >= (int64_t)H * D,
                "gmd_attention_ip: row stride smaller than H*D");
    AttnIpParams p;
    p.Q = (const bf16_t*)Q; p.K = (const bf16_t*)K; p.Vt = (const bf16_t*)Vt; p.Kip = (const bf16_t*)Kip; p.Vtip = (const bf16_t*)Vtip;
    p.O = (bf16_t*)O;
    p.ip_scale = ip_scale + ip_scale_index;
    p.Nq = Nq; p.Nk = Nk; p.Nip = Nip; p.H = H;
    p.ldq = ldq; p.ldk = ldk; p.ldvt = ldvt; p.ldkip = ldkip; p.ldvtip = ldvtip; p.ldo = ldo;
    p.sQ = strideQ; p.sK = strideK; p.sVt = strideVt; p.sKip = strideKip; p.sVtip = strideVtip; p.sO = strideO;
    p.scale_log2 = softmax_scale * 1.4426950408889634f;
    hipStream_t s = (hipStream_t)stream;
    return dtype == GMD_F16 ? dispatch_attn_ip<f16_t>(p, B, H, D, s) : dispatch_attn_ip<bf16_t>(p, B, H, D, s);
}

GMD_WG_TRACE_SETTER(attention_ip)
