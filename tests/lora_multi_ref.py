"""Several LoRA adapters at once: plain helper module beside tests/lora_ref.py and tests/lora_ff_ref.py, which it reuses by import.
Operands of the stacked launch (factors side by side along the rank, a DIFFERENT scale on every column), a torch emulation of its
contract, its per-element bound (``stacked_ref_bound``: lora_ref.update_ref_bound extended term by term), the bound of the
sequential route (one single-adapter update after the other), and merged / hooked CPU oracles for a SET of weighted adapters."""
import copy

import torch
import torch.nn.functional as F

import lora_ff_ref as FR
import lora_ref as R
import parity as P


def pad(n, m):
    return (n + m - 1) // m * m


def column_ranges(ranks):
    out, c = [], 0
    for r in ranks:
        out.append((c, c + r))
        c += r
    return out


def column_scales(rp, rank_sum, seed):
    """float32 [rp]: every column a DIFFERENT value, mixed signs, magnitudes 0.1 ... 2 (a mis-indexed scale cannot pass); the pad
    columns [rank_sum, rp) hold 1e4, which zero factor rows must keep out of the result."""
    g = torch.Generator().manual_seed(seed)
    mag = 0.1 + 1.9 * (torch.randperm(rp, generator=g).double() + 0.5) / rp  # distinct by construction
    sign = torch.where(torch.arange(rp) % 3 == 1, -1.0, 1.0).double()
    cs = (mag * sign).to(torch.float32)
    cs[rank_sum:] = 1.0e4
    assert len(set(cs[:rank_sum].tolist())) == rank_sum
    return cs


def stacked_operands(M, K, ranks, N, dtype, seed):
    """x [M, K]; a [Rp, K], b [N, Rp]: the adapters of ``ranks`` packed tightly, the SUM zero-padded to a multiple of 32; y0 [M, N];
    cs [Rp] (column_scales).  CPU tensors holding values of ``dtype`` (cs: float32).  By construction |cs * T| stays far inside
    float16's range: |T| is ~1, |cs| <= 2 on the real columns (asserted)."""
    g = torch.Generator().manual_seed(seed)
    total = sum(ranks)
    rp = pad(total, 32)
    x = torch.randn(M, K, generator=g).to(dtype)
    a, b = torch.zeros(rp, K), torch.zeros(N, rp)
    for r, (c0, c1) in zip(ranks, column_ranges(ranks)):
        a[c0:c1] = torch.randn(r, K, generator=g) / K ** 0.5
        b[:, c0:c1] = torch.randn(N, r, generator=g) / (r * len(ranks)) ** 0.5
    y0 = torch.randn(M, N, generator=g).to(dtype)
    a, b = a.to(dtype), b.to(dtype)
    cs = column_scales(rp, total, seed + 1)
    st = (cs.double()[None, :total] * (x.double() @ a.double().T)[:, :total]).abs().max() if M else 0.0
    assert float(st) < 64.0, f"|s T| = {float(st)} is not far inside float16's range"
    return x, a, b, y0, cs


def emulate(x, a, b, y, cs, dtype):
    """The contract in torch: float32 accumulation, the column scale in float32 in front of That's ONE rounding, one rounding on the
    store."""
    that = (cs.float()[None, :] * (x.float() @ a.float().T)).to(dtype)
    return (y.float() + that.float() @ b.float().T).to(dtype)


def _stacked_pre(x, a, b, y, cs, dtype):
    """(float64 y + U, its error before the store's rounding): lora_ref.update_ref_bound term by term, with
      1. first product T = x a^T: unchanged;
      2'. the column scale multiplies the float32 accumulator ONCE in front of the rounding: s_j (T + e1) rounded in float32,
          U_F32 |s_j| (|T| + e1); then the ONE rounding of s_j T to ``dtype``;
      3. second product: float32 accumulation of Rp products of |That| with |b|: unchanged;
      4'. NO scale behind the second product: the term is gone;
      5. the add to float(y) rounds once in float32."""
    u = P.unit_roundoff(dtype)
    x64, a64, b64, y64 = (t.to(torch.float64) for t in (x, a, b, y))
    s = cs.to(torch.float64)[None, :]
    K, Rp = a.shape[1], a.shape[0]
    T = x64 @ a64.T
    e1 = P.accumulate_bound(x64.abs() @ a64.abs().T, K, height=P.mfma_height(K, 32))
    sT = s * T
    es = s.abs() * e1 + P.U_F32 * s.abs() * (T.abs() + e1)          # 2'. the float32 product
    eT = es + u * (sT.abs() + es) + P._TINY[dtype]                  #     the ONE rounding of That
    U = sT @ b64.T  # (a zero-padded column: T = e1 = 0 and b's column is 0, so it adds nothing here whatever its scale)
    absU = (sT.abs() + eT) @ b64.abs().T
    eU = eT @ b64.abs().T + P.accumulate_bound(absU, Rp, height=P.mfma_height(Rp, 32))
    value = y64 + U
    e = eU + P.U_F32 * (y64.abs() + U.abs() + eU)                   # 5.
    return value, e


def stacked_ref_bound(x, a, b, y, cs, dtype):
    """(float64 reference, per-element bound) of the stacked update ``y + ((x a^T) * cs) b^T`` (_stacked_pre, then the ONE rounding
    of the stored value)."""
    value, e = _stacked_pre(x, a, b, y, cs, dtype)
    return value, P._finish(value, e, dtype)


def stacked_geglu_ref_bound(x, a, b, y, cs, dtype):
    """(float64 F, bound) of ``geglu(y + ((x a^T) * cs) b^T)`` over the INTERLEAVED layout: _stacked_pre for v and g (NOT rounded to
    ``dtype``), then terms 6 and 7 of lora_ff_ref.geglu_update_ref_bound."""
    u = P.unit_roundoff(dtype)
    pre, e = _stacked_pre(x, a, b, y, cs, dtype)
    (v, g), (ev, eg) = FR.deinterleave_cols(pre), FR.deinterleave_cols(e)
    gel = F.gelu(g)
    dg = P.LIP_GELU * eg + FR._gelu_erf_eval_error(g)
    out = v * gel
    eo = gel.abs() * ev + v.abs() * dg + ev * dg
    eo = eo + P.U_F32 * (out.abs() + eo)
    return out, eo + u * (out.abs() + eo) + P._TINY[dtype]


def split_parts(a, b, cs, ranks, multiple):
    """The stacked operands taken apart again: [(a_i [pad(r_i), K], b_i [N, pad(r_i)])] per adapter, zero-padded to ``multiple``.
    (The sequential route has ONE scalar per adapter, so its tests use per-adapter scalars, not ``cs``.)"""
    out = []
    for r, (c0, c1) in zip(ranks, column_ranges(ranks)):
        rp = pad(r, multiple)
        ai, bi = torch.zeros(rp, a.shape[1], dtype=a.dtype), torch.zeros(b.shape[0], rp, dtype=b.dtype)
        ai[:r], bi[:, :r] = a[c0:c1], b[:, c0:c1]
        out.append((ai, bi))
    return out


def sequential_ref_bound(x, parts, scalars, y, dtype, one):
    """(float64 reference, bound) of one single-adapter update after the other, Y ROUNDED to ``dtype`` in between.  ``one(x, a, b, y,
    s)`` is the single update's (reference, bound) -- lora_ref.update_ref_bound or update_ref_bound_f32 -- applied per adapter to the
    running float64 reference.  The next update reads a y that is off its reference by <= the bound so far; its own bound depends on
    y only through U_F32 |y| and u |value|, so what came before enters as bound_prev (1 + 2 u)."""
    u = P.unit_roundoff(dtype)
    ref, bound = y.to(torch.float64), torch.zeros(y.shape, dtype=torch.float64)
    for (a, b), s in zip(parts, scalars):
        ref, bi = one(x, a, b, ref, s)
        bound = bound * (1 + 2 * u) + bi
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------------
# oracles for a SET of weighted adapters: [(canon, weight)], canon = {module: (A, B, alpha)} over any of the twelve targets
# ---------------------------------------------------------------------------------------------------------------------------
def merged_oracle(ou, adapters, scale=1.0):
    """W + sum_a s w_a f_a B_a A_a, the sum formed in float64 and rounded ONCE into a copy of the oracle."""
    m = copy.deepcopy(ou)
    mods = FR.target_modules(m)
    delta = {}
    for canon, w in adapters:
        for name, (a, b, alpha) in canon.items():
            d = scale * w * R._factor(a, alpha) * (b.double() @ a.double())
            delta[name] = delta.get(name, 0) + d
    with torch.no_grad():
        for name, d in delta.items():
            wt = mods[name].weight
            wt.copy_((wt.double() + d.reshape(wt.shape)).to(wt.dtype))
    return m


def hooked_oracle(ou, adapters, scale=1.0):
    """The weights untouched; every adapter adds its own update at run time (lora_ff_ref.hooked_oracle once per adapter)."""
    m = copy.deepcopy(ou)
    mods = FR.target_modules(m)
    for canon, w in adapters:
        for name, (a, b, alpha) in canon.items():
            f = scale * w * R._factor(a, alpha)
            conv = mods[name].weight.dim() == 4

            def hook(mod, inp, out, a=a, b=b, f=f, conv=conv):
                x = inp[0]
                if conv:
                    x = x.permute(0, 2, 3, 1)
                upd = f * ((x @ a.T.to(x.dtype)) @ b.T.to(x.dtype))
                return out + (upd.permute(0, 3, 1, 2) if conv else upd)

            mods[name].register_forward_hook(hook)
    return m
