"""Integer oracle of the fused ResNet-20 kernels (csrc/kernels/resnet*.hip), ONE kernel at a time: the
3x3 convolution at stride 1 / 2 with its input and weight gradients, the BatchNorm prologue / epilogue
coefficients, the option-A shortcut and its gradient, the per-image split-K slabs, both bf16 weight
shadows and the head.  Plain torch on the CPU in fp64, written from the definitions in
csrc/kernels/api_resnet.h and models/resnet.py; no project kernel and no model function is called.

Why it is exact although BatchNorm is involved: every kernel takes its statistics slots, gamma and
beta as INPUT tensors, so a case chooses them.  With N = nvalid * H * H a power of two, an integer mean
k_c and t_c in {1, 0.25} the slots are written so that sum = N k_c and sum of squares =
N (k_c^2 + t_c - eps); the kernels then get mean == k_c and rstd == 1.0f or 2.0f exactly (the fp64
value is within 1e-12 of 1 or 2, its cast to float cannot land elsewhere), and with integer gamma, beta
and reduction totals R = N r every coefficient of the forward (sc, sh) and of the backward (A, Bc, Cc)
is a small integer.  From there on it is tests/exact_ref.py again: every value stored as bf16 is an
integer of |v| <= 256, every bf16 x bf16 product is exact in fp32 and every fp32 sum is exact while the
sum of |terms| stays below 2^24, in any summation order, MFMA included.  A correct kernel reproduces
this oracle bit for bit; the fixed-point statistics are exact by design, so their decoded totals equal
the oracle's integer sums and every fraction word is zero.

Layouts: activations NHWC, weights HWIO (models/resnet.py).  Every function computes in fp64 and takes
real inputs too (the CPU tests compare them with autograd on random reals); ``_int`` asserts that a
result is an integer tensor.
"""
import functools
import types

import torch

F64 = torch.float64
BN_EPS = 1e-3                  # models/resnet.py BN_EPS, rn_stats.h BN_EPS
NSLOT = 8                      # statistics slots per layer
FX_ONE = float(2 ** 48)        # fraction unit of the fixed-point statistics
LIM = 2 ** 24                  # fp32 sums of integers are exact below this
BF16_MAX = 256                 # bf16 holds every integer up to here

# the six conv geometries (cin, cout, hin, stride)
STEM, S16, D32 = (3, 16, 32, 1), (16, 16, 32, 1), (16, 32, 32, 2)
S32, D64, S64 = (32, 32, 16, 1), (32, 64, 16, 2), (64, 64, 8, 1)
GEOMS = (STEM, S16, D32, S32, D64, S64)


def _int(t):
    r = t.round()
    assert torch.equal(r, t), "not an integer tensor"
    return r.to(torch.int64)


def cinp(cin):
    return max(cin, 8)


def kp(cin):
    return (9 * cinp(cin) + 31) // 32 * 32


def kpd(cout):
    return (9 * cout + 31) // 32 * 32


# --------------------------------------------------------------------------------------------------
# convolution: z[b, y, x, co] = sum_{kh, kw, ci} xpad[b, s y + kh, s x + kw, ci] w[kh, kw, ci, co],
# xpad = x padded by (1, 1) at stride 1 and by (0, 1) at stride 2 (TF SAME on even sizes)
def _pad_before(stride):
    return 1 if stride == 1 else 0


def _xpad(x, stride):
    B, H, W, C = x.shape
    pb = _pad_before(stride)
    out = torch.zeros(B, H + pb + 1, W + pb + 1, C, dtype=F64)
    out[:, pb:pb + H, pb:pb + W, :] = x
    return out


def _tap(t, kh, kw, stride, hout):
    return t[:, kh:kh + stride * hout:stride, kw:kw + stride * hout:stride, :]


def conv3x3(x, w, stride):
    x, w = x.to(F64), w.to(F64)
    hout = x.shape[1] // stride
    xp = _xpad(x, stride)
    z = torch.zeros(x.shape[0], hout, hout, w.shape[3], dtype=F64)
    for kh in range(3):
        for kw in range(3):
            z += torch.einsum("byxi,io->byxo", _tap(xp, kh, kw, stride, hout), w[kh, kw])
    return z


def conv3x3_dgrad(g, w, stride):
    """Input gradient [B, hin, hin, CIN] of the output gradient ``g`` [B, hout, hout, COUT]: every
    output pixel scatters g w[kh, kw] to the padded input cell it read."""
    g, w = g.to(F64), w.to(F64)
    hout = g.shape[1]
    hin = hout * stride
    pb = _pad_before(stride)
    gp = torch.zeros(g.shape[0], hin + pb + 1, hin + pb + 1, w.shape[2], dtype=F64)
    for kh in range(3):
        for kw in range(3):
            _tap(gp, kh, kw, stride, hout).add_(torch.einsum("byxo,io->byxi", g, w[kh, kw]))
    return gp[:, pb:pb + hin, pb:pb + hin, :].contiguous()


def conv3x3_wgrad(x, g, stride):
    """Per-image weight-gradient contributions [B, 9, CINP, COUT] (tap = 3 kh + kw; rows ci >= CIN of the
    stem are zero): sum any grouping of images over dim 0."""
    x, g = x.to(F64), g.to(F64)
    B, cin, hout = x.shape[0], x.shape[3], g.shape[1]
    xp = _xpad(x, stride)
    out = torch.zeros(B, 9, cinp(cin), g.shape[3], dtype=F64)
    for kh in range(3):
        for kw in range(3):
            out[:, 3 * kh + kw, :cin, :] = torch.einsum("byxi,byxo->bio", _tap(xp, kh, kw, stride, hout), g)
    return out


# --------------------------------------------------------------------------------------------------
# BatchNorm coefficients from the statistics TOTALS (rn_stats.h bn_mean_rstd / bnb_coeffs)
def bn_coeffs(stat, red, gamma, N, f32=False):
    """``stat`` = (sum z, sum z^2), ``red`` = (R1 = sum g_y, R2 = sum g_y xhat) or None, per channel,
    over N elements.  Returns (mean, rstd, A, Bc, Cc): y = gamma rstd (z - mean) + beta forward,
    g_z = A g_y + Bc z + Cc backward with A = gamma rstd, Bc = -A rstd R2 / N, Cc = -A R1 / N - Bc mean.
    ``f32``: mean and rstd rounded to float as the kernels keep them (exact cases: a no-op by
    construction, which make_case asserts)."""
    s1, s2, gamma = stat[0].to(F64), stat[1].to(F64), gamma.to(F64)
    mean = s1 / N
    var = (s2 / N - mean * mean).clamp(min=0)
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    if f32:
        mean, rstd = mean.float().double(), rstd.float().double()
    A = gamma * rstd
    if red is None:
        return mean, rstd, A, None, None
    r1, r2 = red[0].to(F64) / N, red[1].to(F64) / N
    Bc = -A * rstd * r2
    Cc = -A * r1 - Bc * mean
    return mean, rstd, A, Bc, Cc


# --------------------------------------------------------------------------------------------------
# option-A shortcut (mode 1 identity, mode 2 subsample + zero upper channels) and its gradient
def shortcut(src, mode):
    if mode == 0:
        return 0.0
    src = src.to(F64)
    if mode == 1:
        return src
    sub = src[:, ::2, ::2, :]
    return torch.cat([sub, torch.zeros_like(sub)], dim=3)


def shortcut_grad(gy_sc, mode):
    """Gradient the shortcut sends to the block input.  Mode 2: gy_sc is [B, H/2, H/2, 2 CIN]; cell
    (y/2, x/2), channels c < CIN, lands on the even (y, x) of [B, H, H, CIN] only."""
    if mode == 0:
        return 0.0
    gy_sc = gy_sc.to(F64)
    if mode == 1:
        return gy_sc
    B, hb, _, c2 = gy_sc.shape
    out = torch.zeros(B, 2 * hb, 2 * hb, c2 // 2, dtype=F64)
    out[:, ::2, ::2, :] = gy_sc[..., :c2 // 2]
    return out


# --------------------------------------------------------------------------------------------------
# one launch each
def fwd_exact(w, stride, nvalid, x=None, z_prev=None, mean=None, rstd=None, gamma=None, beta=None, sc_src=None,
              sc_mode=0):
    """rn_fwd: a_out = relu(gamma rstd (z_prev - mean) + beta + shortcut) (None for the stem, whose input
    ``x`` is the gathered pixels), z = conv(a_out) for ALL images, and the per-channel sum z / sum z^2
    over the images b < nvalid."""
    a_out = None
    if x is None:
        sc = gamma.to(F64) * rstd
        sh = beta.to(F64) - mean * sc
        a_out = (z_prev.to(F64) * sc + sh + shortcut(sc_src, sc_mode)).clamp(min=0)
        x = a_out
    z = conv3x3(x, w, stride)
    return a_out, z, z[:nvalid].sum((0, 1, 2)), (z[:nvalid] ** 2).sum((0, 1, 2))


def gz_exact(gy, z, A, Bc, Cc, nvalid):
    """g_z of layer l as the dgrad / wgrad prologues rebuild it; exactly 0 for the padding images."""
    g = A * gy.to(F64) + Bc * z.to(F64) + Cc
    g[nvalid:] = 0
    return g


def dgrad_exact(gy, z, A, Bc, Cc, w, stride, a_prev, z_prev, mean_prev, rstd_prev, gy_sc, sc_mode, nvalid):
    """rn_dgrad: (g_z, gy_prev = (a_prev > 0) (dgrad(g_z) + shortcut gradient), R1_prev = sum gy_prev,
    R2_prev = sum gy_prev xhat_prev with xhat_prev = (z_prev - mean_prev) rstd_prev)."""
    g_z = gz_exact(gy, z, A, Bc, Cc, nvalid)
    gy_prev = (conv3x3_dgrad(g_z, w, stride) + shortcut_grad(gy_sc, sc_mode)) * (a_prev > 0)
    xhat = (z_prev.to(F64) - mean_prev) * rstd_prev
    return g_z, gy_prev, gy_prev.sum((0, 1, 2)), (gy_prev * xhat).sum((0, 1, 2))


def wgrad_exact(x, g_z, stride):
    """rn_wgrad: per-image slabs [B, 9 CINP, COUT] in the kernel's row order k = tap CINP + ci."""
    c = conv3x3_wgrad(x, g_z, stride)
    return c.reshape(c.shape[0], 9 * c.shape[2], c.shape[3])


def slab_sums(slabs, G):
    """Per-group slabs [G, 9 CINP, COUT]: group grp holds images [grp B / G, (grp + 1) B / G)."""
    B = slabs.shape[0]
    return torch.stack([slabs[g * B // G:(g + 1) * B // G].sum(0) for g in range(G)])


def shadow_fwd(w):
    """bf16 forward shadow [COUT, KP]: column k = tap CINP + ci, padding columns zero."""
    _, _, cin, cout = w.shape
    out = torch.zeros(cout, kp(cin), dtype=w.dtype)
    for tap in range(9):
        out[:, tap * cinp(cin):tap * cinp(cin) + cin] = w[tap // 3, tap % 3].t()
    return out


def shadow_dgrad(w):
    """bf16 dgrad shadow [CIN, KPD]: column k' = (8 - tap) COUT + co (the kernel rotated by 180
    degrees), padding columns zero."""
    _, _, cin, cout = w.shape
    out = torch.zeros(cin, kpd(cout), dtype=w.dtype)
    for tap in range(9):
        out[:, (8 - tap) * cout:(9 - tap) * cout] = w[tap // 3, tap % 3]
    return out


def head_exact(z, mean, rstd, gamma, beta, sc, fcw, fcb, labels, inv_batch, nvalid):
    """rn_head: av = relu(bn(z) + sc), pooled = sum over the 64 pixels / 64, logits = pooled fcw + fcb
    (exact: multiples of 1/64), first-maximum prediction; in fp64 the per-image loss, dlogits =
    (softmax - onehot) inv_batch, dW_fc = pooled (x) dlogits, db_fc = dlogits, gpool = dlogits fcw^T /
    64, g_y = (av > 0) gpool and its reductions.  Padding images (b >= nvalid): loss, correct, dlogits
    and g_y are zero; their logits are still computed."""
    z, sc, fcw, fcb = z.to(F64), sc.to(F64), fcw.to(F64), fcb.to(F64)
    B = z.shape[0]
    s = gamma.to(F64) * rstd
    av = (z * s + (beta.to(F64) - mean * s) + sc).clamp(min=0)
    pooled = av.sum((1, 2)) / 64
    logits = pooled @ fcw + fcb
    m = logits.max(1, keepdim=True).values
    pred = torch.where(logits == m, torch.arange(10), 10).min(1).values
    real = (torch.arange(B) < nvalid)
    lse = m[:, 0] + torch.log(torch.exp(logits - m).sum(1))
    lab = labels.long()
    loss = (lse - logits[torch.arange(B), lab]) * real
    onehot = torch.zeros(B, 10, dtype=F64)
    onehot[torch.arange(B), lab] = 1
    prob = torch.softmax(logits, 1)
    dlogits = (prob - onehot) * inv_batch * real[:, None]
    gpool = dlogits @ fcw.t() / 64
    mask = av > 0
    gy = mask * gpool[:, None, None, :]
    xhat = (z - mean) * rstd
    return types.SimpleNamespace(av=av, pooled=pooled, logits=logits, pred=pred, loss=loss, prob=prob, dlogits=dlogits,
                                 correct=((pred == lab) & real).long(), dW=pooled[:, :, None] * dlogits[:, None, :],
                                 gpool=gpool, mask=mask, gy=gy, xhat=xhat, R1=gy.sum((0, 1, 2)),
                                 R2=(gy * xhat).sum((0, 1, 2)), tie=(logits == m).sum(1) > 1)


# --------------------------------------------------------------------------------------------------
# fixed-point statistics slots (host mirror of rn_stats.h fx_add / fx_total, written here from the
# header's description: int64 integer part at [e], 48-bit fraction at [128 + e], 8 slots per layer)
def fx_split(x):
    x = x.to(F64)
    f = torch.floor(x)
    return f.long(), torch.round((x - f) * FX_ONE).long()


def encode_slots(t1, t2, gen):
    """Slots [NSLOT, 256] int64 whose totals are ``t1`` at [0, C) and ``t2`` at [64, 64 + C): every
    total is spread over all 8 slots with signed integer parts that cancel, and 0..3 whole units are
    moved from the integer words into the fraction words, so the consumer's slot summation and its
    fraction carry both decide the result."""
    C = t1.numel()
    slots = torch.zeros(NSLOT, 256, dtype=torch.int64)
    for base, tot in ((0, t1), (64, t2)):
        hi, lo = fx_split(tot)
        carry = torch.randint(0, 4, (C,), generator=gen)
        hi, lo = hi - carry, lo + carry * 2 ** 48
        h = torch.randint(-(2 ** 20), 2 ** 20, (NSLOT, C), generator=gen)
        h[NSLOT - 1] = hi - h[:NSLOT - 1].sum(0)
        frac = torch.rand(NSLOT, C, generator=gen, dtype=F64)
        lp = torch.floor(frac / frac.sum(0) * lo.double()).long()
        lp[0] += lo - lp.sum(0)
        assert bool((lp >= 0).all())
        slots[:, base:base + C] = h
        slots[:, 128 + base:128 + base + C] = lp
    return slots


def fx_total(slots):
    """Decoded totals fp64 [128] of slots [NSLOT, 256], as rn_stats.h fx_total forms them."""
    return slots[:, :128].sum(0).double() + slots[:, 128:].sum(0).double() * (1.0 / FX_ONE)


def emulate_mean_rstd(slots, C, inv_n):
    """rn_stats.h bn_mean_rstd on the CPU: fp64 arithmetic without contraction, float results."""
    tot = fx_total(slots)
    inv = float(torch.tensor(inv_n, dtype=torch.float32))
    m = tot[:C] * inv
    var = (tot[64:64 + C] * inv - m * m).clamp(min=0)
    return m.float(), (1.0 / torch.sqrt(var + BN_EPS)).float()


def stat_totals(mean, rstd, N):
    """The (sum, sum of squares) that give integer ``mean`` and rstd in {1, 2} over N elements."""
    t = 1.0 / (rstd.to(F64) ** 2)
    return N * mean.to(F64), N * (mean.to(F64) ** 2 + t - BN_EPS)


# --------------------------------------------------------------------------------------------------
# cases
# weight density (fraction of +-1 taps) per (kind, geometry): |z| and |g_a| have to stay <= 256 with
# up to 576 taps per output
DENSITY = {("fwd", STEM): 1.0, ("fwd", S16): 0.12, ("fwd", D32): 0.12, ("fwd", S32): 0.06, ("fwd", D64): 0.06,
           ("fwd", S64): 0.03,
           ("bwd", STEM): 1.0, ("bwd", S16): 0.12, ("bwd", D32): 0.10, ("bwd", S32): 0.06, ("bwd", D64): 0.05,
           ("bwd", S64): 0.03}


def _bf16_int(name, t):
    assert int(t.abs().max()) <= BF16_MAX, f"{name} leaves the bf16 integers: {int(t.abs().max())}"
    return t


class _Rng:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def ints(self, lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=self.g)

    def pick(self, values, *shape):
        v = torch.tensor(values)
        return v[torch.randint(0, len(values), shape, generator=self.g)]

    def sparse_pm1(self, density, *shape):
        keep = torch.rand(*shape, generator=self.g) < density
        return keep * (2 * self.ints(0, 1, *shape) - 1)


def _bn_inputs(r, C, N):
    """Integer mean in -2..2, rstd in {1, 2} (both values present), their slots."""
    mean = r.ints(-2, 2, C)
    rstd = r.pick([1, 2], C)
    rstd[0], rstd[1] = 1, 2
    s1, s2 = stat_totals(mean, rstd, N)
    return mean.double(), rstd.double(), encode_slots(s1, s2, r.g), (s1, s2)


@functools.lru_cache(maxsize=None)
def make_case(kind, geom, seed, B, nvalid, sc_mode):
    """Seeded small-integer inputs of ONE launch plus every oracle result (cached: treat as read-only).
    ``kind``: "fwd" (rn_fwd of ``geom`` with forward shortcut mode ``sc_mode``), "bwd" (rn_dgrad /
    rn_wgrad / rn_bwd of ``geom`` with backward shortcut mode ``sc_mode``; the stem has a wgrad only) or
    "head".  The preconditions are asserted from the oracle alone."""
    if kind == "head":
        return _make_head(seed, B, nvalid)
    cin, cout, hin, stride = geom
    r = _Rng(seed)
    w = r.sparse_pm1(DENSITY[kind, geom], 3, 3, cin, cout)
    c = types.SimpleNamespace(kind=kind, geom=geom, B=B, nvalid=nvalid, sc_mode=sc_mode, w=w, seed=seed)
    if cin == 3:
        c.data = r.ints(0, 3, 64, 32, 32, 3).to(torch.uint8)
        c.idx = torch.randperm(64, generator=r.g)[:B].to(torch.int32)
        x = c.data[c.idx.long()].double()
    return (_make_fwd if kind == "fwd" else _make_bwd)(c, r, x if cin == 3 else None)


def _make_fwd(c, r, x):
    cin, cout, hin, stride = c.geom
    B, nvalid = c.B, c.nvalid
    if x is None:
        N = nvalid * hin * hin
        c.N_prev = N
        c.z_prev = r.ints(-2, 2, B, hin, hin, cin)
        c.mean, c.rstd, c.stat_prev, c.stat_prev_totals = _bn_inputs(r, cin, N)
        c.gamma = r.pick([-2, -1, 1, 2], cin).float()
        c.beta = r.ints(-2, 2, cin).float()
        c.sc_src = None
        if c.sc_mode == 1:
            c.sc_src = r.ints(0, 3, B, hin, hin, cin)
        elif c.sc_mode == 2:
            c.sc_src = r.ints(0, 3, B, 2 * hin, 2 * hin, cin // 2)
        a_out, z, s1, s2 = fwd_exact(c.w, stride, nvalid, z_prev=c.z_prev, mean=c.mean, rstd=c.rstd, gamma=c.gamma,
                                     beta=c.beta, sc_src=c.sc_src, sc_mode=c.sc_mode)
        c.a_out = _bf16_int("a_out", _int(a_out))
        zero = float((c.a_out == 0).double().mean())
        assert 0.2 <= zero <= 0.8, f"the ReLU zeroes {zero:.0%} of a_out"
        if c.sc_mode == 2:
            assert bool(c.sc_src[:, ::2, ::2].any()) and bool(c.sc_src[:, 1::2].any()) and bool(c.sc_src[:, :, 1::2].any())
        xin = c.a_out
    else:
        a_out, z, s1, s2 = fwd_exact(c.w, stride, nvalid, x=x)
        c.a_out, xin = None, _int(x)
    c.z, c.s1, c.s2 = _bf16_int("z", _int(z)), _int(s1), _int(s2)
    # every fp32 sum of the launch: a conv output, a per-image per-channel statistic partial
    assert float(conv3x3(xin.abs(), c.w.abs(), stride).max()) < LIM
    assert float((z ** 2).sum((1, 2)).max()) < LIM and float(z.abs().sum((1, 2)).max()) < LIM
    if stride == 2:                       # only the last input row / column meets the padded tap
        assert bool(xin[:, hin - 1].any()) and bool(xin[:, :, hin - 1].any())
        assert bool(c.w[2].any()) and bool(c.w[:, 2].any())
    assert bool(c.z[nvalid:].any()) or nvalid == B, "padding images must still be computed"
    return c


def _make_bwd(c, r, x):
    cin, cout, hin, stride = c.geom
    B, nvalid = c.B, c.nvalid
    hout = hin // stride
    N = nvalid * hout * hout
    c.N = N
    c.gy = r.ints(-3, 3, B, hout, hout, cout)
    c.gy[nvalid:] = 0                     # as the head and the earlier dgrads leave the padding images
    c.z = r.ints(-2, 2, B, hout, hout, cout)
    c.mean, c.rstd, c.stat, c.stat_totals = _bn_inputs(r, cout, N)
    c.gamma = r.pick([-2, -1, 1, 2], cout).float()
    c.r1, c.r2 = r.ints(-2, 2, cout), r.ints(-1, 1, cout)
    c.red_totals = (N * c.r1.double(), N * c.r2.double())
    c.red = encode_slots(*c.red_totals, r.g)
    _, _, A, Bc, Cc = bn_coeffs(c.stat_totals, c.red_totals, c.gamma, N, f32=True)
    c.A, c.Bc, c.Cc = _int(A), _int(Bc), _int(Cc)
    assert bool(c.Bc.any()) and bool(c.Cc.any())
    if x is None:
        c.N_prev = nvalid * hin * hin
        c.a_prev = r.ints(0, 3, B, hin, hin, cin) * (torch.rand(B, hin, hin, cin, generator=r.g) < 0.6)
        c.z_prev = r.ints(-2, 2, B, hin, hin, cin)
        c.mean_prev, c.rstd_prev, c.stat_prev, c.stat_prev_totals = _bn_inputs(r, cin, c.N_prev)
        c.gy_sc = None
        if c.sc_mode == 1:
            c.gy_sc = r.ints(-3, 3, B, hin, hin, cin)
        elif c.sc_mode == 2:
            c.gy_sc = r.ints(-3, 3, B, hin // 2, hin // 2, 2 * cin)
        if c.gy_sc is not None:
            c.gy_sc[nvalid:] = 0
        g_z, gy_prev, R1, R2 = dgrad_exact(c.gy, c.z, A, Bc, Cc, c.w, stride, c.a_prev, c.z_prev, c.mean_prev,
                                           c.rstd_prev, c.gy_sc, c.sc_mode, nvalid)
        c.gy_prev, c.R1_prev, c.R2_prev = _bf16_int("gy_prev", _int(gy_prev)), _int(R1), _int(R2)
        xin = c.a_prev
        # fp32 sums of the dgrad: an input-gradient element, the per-image reduction partials
        assert float(conv3x3_dgrad(g_z.abs(), c.w.abs(), stride).max()) + 3 < LIM
        xhat = (c.z_prev.double() - c.mean_prev) * c.rstd_prev
        assert float((gy_prev * xhat).abs().sum((1, 2)).max()) < LIM and float(gy_prev.abs().sum((1, 2)).max()) < LIM
        zero = float((c.a_prev == 0).double().mean())
        assert 0.2 <= zero <= 0.8
        assert not bool(c.gy_prev[nvalid:].any())
        if nvalid < B:
            assert bool(c.a_prev[nvalid:].any()) and bool(c.z_prev[nvalid:].any())
    else:
        g_z = gz_exact(c.gy, c.z, A, Bc, Cc, nvalid)
        xin = _int(x)
    c.g_z = _bf16_int("g_z", _int(g_z))
    for name, edge in (("top row", c.g_z[:nvalid, 0]), ("bottom row", c.g_z[:nvalid, -1]),
                       ("left column", c.g_z[:nvalid, :, 0]), ("right column", c.g_z[:nvalid, :, -1])):
        assert float((edge != 0).double().mean()) >= 0.05, f"g_z is nearly zero in its {name}"
    c.slabs = _int(wgrad_exact(xin, g_z, stride))
    # every fp32 sum of the wgrad: a slab element over ALL images bounds every group and every order
    assert float(wgrad_exact(xin.abs(), g_z.abs(), stride).sum(0).max()) < LIM
    assert bool(c.slabs.any())
    if cin == 3:
        assert not bool(c.slabs.view(B, 9, 8, cout)[:, :, 3:].any())
    if stride == 2:
        assert bool(xin[:, hin - 1].any()) and bool(xin[:, :, hin - 1].any())
    if nvalid < B:
        assert bool(c.z[nvalid:].any()) and bool(xin[nvalid:].any()) and not bool(c.slabs[nvalid:].any())
    return c


def _make_head(seed, B, nvalid):
    r = _Rng(seed)
    c = types.SimpleNamespace(kind="head", B=B, nvalid=nvalid, seed=seed, N=nvalid * 64)
    # a per-image level under the pixel noise in a quarter of the channels: the pooled vectors (so the
    # predictions) differ by image, yet the logits stay within a few units of each other
    c.z = r.ints(-1, 1, B, 8, 8, 64) + r.ints(-1, 1, B, 1, 1, 64) * (r.ints(0, 3, 1, 1, 1, 64) == 0)
    c.mean, c.rstd, c.stat, c.stat_totals = _bn_inputs(r, 64, c.N)
    c.gamma = r.pick([-2, -1, 1, 2], 64).float()
    c.beta = r.ints(-2, 2, 64).float()
    c.sc = r.ints(0, 3, B, 8, 8, 64)
    # integer fc weights, a few +-1 per class; classes 7 and 8 repeat classes 2 and 4, so the top two
    # logits of an image whose best class is one of them tie and the first-maximum rule decides
    # (every channel feeds one or two classes, so no pooled gradient is exactly zero and the zero
    # pattern of g_y is the av > 0 mask alone)
    c.fcw = torch.zeros(64, 10)
    free = [0, 1, 2, 3, 4, 5, 6, 9]
    c.fcw[torch.arange(64), r.pick(free, 64)] = (2 * r.ints(0, 1, 64) - 1).float()
    second = r.ints(0, 1, 64).bool()
    c.fcw[torch.arange(64)[second], r.pick(free, 64)[second]] = (2 * r.ints(0, 1, 64) - 1).float()[second]
    c.fcw[:, 7], c.fcw[:, 8] = c.fcw[:, 2], c.fcw[:, 4]
    c.inv_batch = 1.0 / nvalid
    c.idx = torch.randperm(64, generator=r.g)[:B].to(torch.int32)
    # the integer bias centres every class on the batch (a condition on the inputs, like the labels):
    # no softmax row saturates and no exponential underflows
    probe = head_exact(c.z, c.mean, c.rstd, c.gamma, c.beta, c.sc, c.fcw, torch.zeros(10), torch.zeros(B, dtype=torch.int64),
                       c.inv_batch, nvalid)
    c.fcb = (-probe.logits.mean(0).round() + r.ints(-1, 1, 10)).float()
    c.fcb[7], c.fcb[8] = c.fcb[2], c.fcb[4]
    probe = head_exact(c.z, c.mean, c.rstd, c.gamma, c.beta, c.sc, c.fcw, c.fcb, torch.zeros(B, dtype=torch.int64),
                       c.inv_batch, nvalid)
    # labels (conditions on the inputs): the first tied image gets the LATER of its tied classes (a
    # last-maximum rule would call it correct), the other tied images and every second image the
    # predicted class, the rest the class after it -- unless that would saturate the softmax row
    lab = torch.zeros(B, dtype=torch.int64)
    first_tie = True
    for b in range(B):
        p = int(probe.pred[b])
        if bool(probe.tie[b]) and first_tie and b < nvalid:
            lab[b] = max(i for i in range(10) if probe.logits[b, i] == probe.logits[b, p])
            first_tie = False
        elif (bool(probe.tie[b]) or b % 2 == 0) and float(probe.prob[b, p]) <= 0.99:
            lab[b] = p
        else:
            lab[b] = (p + 1) % 10
    c.labels64 = r.ints(0, 9, 64).to(torch.int32)
    c.labels64[c.idx.long()] = lab.to(torch.int32)
    c.labels = lab
    o = head_exact(c.z, c.mean, c.rstd, c.gamma, c.beta, c.sc, c.fcw, c.fcb, lab, c.inv_batch, nvalid)
    c.o = o
    _bf16_int("av", _int(o.av))
    c.logits64 = _int(o.logits * 64)
    assert float((o.pooled.abs() @ c.fcw.abs().double() + c.fcb.abs().double()).max()) * 64 < LIM
    real = torch.arange(B) < nvalid
    assert int((o.tie & real).sum()) >= 2 and int((~o.tie & real).sum()) >= 2, "tied and untied real images"
    assert int(o.correct.sum()) >= 2 and int((real & (o.correct == 0)).sum()) >= 2
    tied_wrong = o.tie & real & (o.correct == 0)
    assert bool(tied_wrong.any()), "no tied image labelled with its later maximum"
    assert float(o.prob[torch.arange(B), lab][:nvalid].max()) <= 0.99, "a saturated softmax row"
    assert bool((o.gpool[:nvalid] != 0).all()), "a pooled gradient is exactly zero"
    assert float((o.logits.max(1).values - o.logits.min(1).values).max()) <= 16, "an exponential below e^-16"
    zero = float((~o.mask).double().mean())
    assert 0.2 <= zero <= 0.8
    return c


# --------------------------------------------------------------------------------------------------
# the (geometry, shortcut mode) pairs of the engine's 19 layers (tests/test_rn_exact_ref.py derives the
# same sets from engine.fused_resnet.LAYERS)
FWD_PAIRS = ((STEM, 0), (S16, 0), (S16, 1), (D32, 1), (S32, 0), (S32, 1), (S32, 2), (D64, 1), (S64, 0), (S64, 1),
             (S64, 2))
BWD_PAIRS = ((S16, 0), (S16, 1), (D32, 2), (S32, 0), (S32, 1), (D64, 2), (S64, 0), (S64, 1))
BWD_DEFAULT_MODE = {STEM: 0, S16: 1, D32: 2, S32: 1, D64: 2, S64: 1}       # the mode of the wgrad / rn_bwd cases

# every case the GPU tests (tests/test_rn_exact_gpu.py) run: (kind, geometry, seed, B, nvalid, sc_mode)
GPU_CASES = (tuple(("fwd", g, 1, 16, 16, m) for g, m in FWD_PAIRS)
             + (("fwd", S16, 2, 16, 8, 1), ("fwd", D64, 2, 16, 8, 1))
             + tuple(("bwd", g, 3, 16, 16, m) for g, m in BWD_PAIRS) + (("bwd", STEM, 3, 16, 16, 0),)
             + (("bwd", S32, 4, 16, 8, 1), ("bwd", D32, 4, 16, 8, 2))
             + (("head", None, 22, 16, 16, 0), ("head", None, 22, 16, 8, 0)))
