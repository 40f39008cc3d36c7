"""Exact-grid cases for the MFMA convolution kernels (tests/test_cpu_conv_exact.py, tests/test_gpu_conv_exact.py).

The argument. An f32 accumulator holds every multiple of a power of two q below 2^24 q exactly. If every term of an
output element (each product x w, the bias, the action bias, the residual) is a multiple of q, and the sum of the
terms' magnitudes stays below 2^24 q, then every partial sum in every order, every MFMA shape and every split is such
a multiple: exact. bf16 x bf16 and fp16 x fp16 products are exact in f32 whatever they are. The only rounding left is
the one correctly rounded store, so a kernel's output must equal the rounded f64 reference bit for bit.

The certificate (`certify`) is that condition, evaluated on the reference side only: per conv, q = (the largest power
of two dividing every activation) x (the largest dividing every weight), lowered to the one dividing every bias /
action bias / residual term: a divisor of every term, never larger than the largest common one, so the condition
checked is the stated one or stricter; and max over the outputs of conv(|x|, |w|) + |bias| + |action bias| + |res|,
in f64, below 2^24 q. A chain is certified conv by conv on the reference's own rounded intermediates. A case that
fails it is a broken case: the generator is to be fixed, never the bound.

Grids. Dense: activations integers in [-3, 3] ([0, 3] for a gathered post-ReLU latent), weights integers in [-2, 2],
small integer biases / tables / residuals; every fourth output channel's bias is moved out to +-[300, 700] so that the
outputs reach the binades where bf16 drops integers: 257 is a tie, 513 is not representable (the 1x1 convs' own sums
never leave +-256). Sparse, for chains, where magnitudes compound: weights in {-1, 0, 1}, m non-zeros per output
channel placed so that every (tap, cin) pair is non-zero for some cout and every cout has every tap; biases are
negative integers. Two-part, for the split-precision f32 convs: one operand i + j 2^-12 (i a non-zero small integer,
j = +-1: 13 significant bits, so the bf16 mid part / the fp16 low part is live), the other single-part integers.

Layouts: references are NCHW f64; `nhwc` gives the kernels' layout. All generators are seeded through
ops_bounds._gen by the case's own parameters."""
import torch
import torch.nn.functional as F

from ops_bounds import _gen

TWO24 = 2.0 ** 24
_SC = 2.0 ** 30          # every grid value is a multiple of 2^-30 (the finest grid here is 2^-12)
BF16, FP16, F32 = torch.bfloat16, torch.float16, torch.float32

MARGINS = {}             # case name -> the smallest 2^24 q / max sum over its convs (printed by the CPU test)


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def lowbit(*ts):
    """The largest power of two that divides every element of every tensor (None entries skipped)."""
    q = None
    for t in ts:
        if t is None:
            continue
        v = t.double().abs() * _SC
        assert torch.equal(v, v.round()) and float(v.max()) < 2.0 ** 62, "value off the 2^-30 grid"
        v = v.to(torch.int64)
        v = v[v != 0]
        if v.numel():
            lb = int((v & -v).min())
            q = lb if q is None else min(q, lb)
    return (int(_SC) if q is None else q) / _SC


def certify(name, bound, q):
    """bound: the f64 tensor of summed magnitudes per output element; q: a power of two dividing every term."""
    m = float(bound.max())
    assert m < TWO24 * q, f"{name}: certificate fails: max sum of magnitudes {m} >= 2^24 q, q = {q}"
    key = name.split("/")[0]
    MARGINS[key] = min(MARGINS.get(key, float("inf")), TWO24 * q / max(m, q))


def rnd(t, dt):
    """The kernel's store: f64 -> f32 is exact under the certificate, f32 -> dt is round-to-nearest-even."""
    f = t.to(F32)
    assert torch.equal(f.double(), t), "reference value not exact in f32"
    return f.to(dt)


def conv_step(name, x, w, bias=None, extra=None, res=None, relu=False):
    """One conv of a case, certified: x [B][Cin][H][W], w [Cout][Cin][ks][ks], bias [Cout], extra / res
    [B][Cout][H][W] (the gathered action-bias rows / the residual). Returns the f64 value the kernel rounds."""
    pad = w.shape[-1] // 2
    terms = [t for t in (None if bias is None else bias.view(1, -1, 1, 1), extra, res) if t is not None]
    q = min([lowbit(x) * lowbit(w)] + [lowbit(t) for t in terms])
    bound = F.conv2d(x.abs(), w.abs(), padding=pad)
    y = F.conv2d(x, w, padding=pad)
    for t in terms:
        bound = bound + t.abs()
        y = y + t
    certify(name, bound, q)
    return torch.relu(y) if relu else y


def tie_stats(pre, dt):
    """(exact ties, non-representable non-ties) among the values `pre` that are rounded to dt."""
    r = pre.to(F32).to(dt).double()
    d = pre - r
    r2 = r + 2.0 * d  # the neighbour on the other side, if pre is the midpoint
    tie = (d != 0) & (r2.to(F32).to(dt).double() == r2)
    return int(tie.sum()), int(((d != 0) & ~tie).sum())


# ------------------------------------------------------------------------------------------------ generators
def dense_w(g, cout, cin, ks):
    return ints(g, (cout, cin, ks, ks), -2, 2)


def tie_bias(g, cout):
    """Small integers; every fourth channel moved to +-[300, 700] (see the module docstring)."""
    b = ints(g, (cout,), -8, 8)
    far = ints(g, (cout,), 300, 700) * (ints(g, (cout,), 0, 1) * 2 - 1)
    return torch.where(torch.arange(cout) % 4 == 1, far, b)


def sparse_w(g, cout, cin, ks, m=16, two_part=False):
    """{-1, 0, 1} weights, m non-zeros per output channel, half of them negative: non-zero k of channel o sits at tap (k + o) % taps and at the
    next unused input channel of that tap (a counter per tap, modulo cin), so each cout has every tap (m >= taps) and
    each (tap, cin) pair is taken once the counters have gone round (cout m / taps >= cin). two_part: the non-zeros are
    i + j 2^-12, i in {+-1, +-2}, j = +-1."""
    taps = ks * ks
    m = max(m, taps, -(-taps * cin // cout))
    # balanced signs per output channel (a shuffled half +1, half -1): on non-negative inputs a channel's sums then
    # centre on zero, so the ReLU cuts about half of EVERY channel, not all of some channels and none of others
    half = torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(-(-m // 2))[:m]
    sign = torch.stack([half[torch.randperm(m, generator=g)] for _ in range(cout)])
    if two_part:
        sign = sign * ints(g, (cout, m), 1, 2) + (ints(g, (cout, m), 0, 1) * 2 - 1) * 2.0 ** -12
    w = torch.zeros(cout, taps, cin, dtype=torch.float64)
    cnt = [0] * taps
    for o in range(cout):
        for k in range(m):
            t = (k + o) % taps
            w[o, t, cnt[t] % cin] = sign[o, k]
            cnt[t] += 1
    return w.view(cout, ks, ks, cin).permute(0, 3, 1, 2).contiguous()


def covers_taps(w):
    """(every (tap, cin) pair non-zero for some cout, every cout non-zero at every tap)."""
    nz = w != 0
    return bool(nz.any(dim=0).all()), bool(nz.any(dim=1).all())


def slots_for(B, S1):
    """Non-monotone slots (2, 0, 1, 5, 3, 4, ...) modulo S1: all S1 in {1, 3, 6} are used once B >= S1."""
    return torch.tensor([((2, 0, 1)[b % 3] + 3 * (b // 3)) % S1 for b in range(B)], dtype=torch.int32)


def acts_for(B, A):
    """Actions 1, 0, 2, 1, ... for A = 3: every action present once B >= A."""
    return torch.tensor([(2 * b + 1) % A for b in range(B)], dtype=torch.int32)


def table_rows(tab, act, H, W):
    """act_bias [HW][A][Cout] gathered per env -> [B][Cout][H][W]."""
    B = act.numel()
    return tab[:, act.long()].permute(1, 2, 0).reshape(B, tab.shape[2], H, W).contiguous()


# ------------------------------------------------------------------------------------------------ towers
# (B, nblocks, gather): towerp has 16 envs per workgroup, the other plans 4 or 8
TOWER_CASES = [(1, 1, 0), (15, 3, 1), (16, 1, 1), (17, 3, 0), (33, 3, 1), (3, 1, 1), (4, 3, 0), (5, 3, 1), (9, 1, 0)]
TOWER_FUSED_CASES = [(16, 0), (17, 0), (16, 1), (17, 1)]  # (B, elem); 2 blocks after the prologue conv


# A chain's input latent: integers in [0, 127] (bf16 holds them). With 16 balanced +-1 weights a conv multiplies the
# magnitudes by about 2, so even a one-block chain ends above 512, where bf16 drops integers (ties, non-representable
# sums); the fp16 image of the fp16 dynamics net (11 bits, range 65504) starts at [0, 63] and ends between 4096 and 2^15.
CHAIN_AMAX = 127


def res_chain(name, x, ws, bs, dt):
    """ResidualBlocks on x (already a dt-valued f64 tensor); returns the last conv's unrounded value."""
    pre = None
    for k in range(len(ws) // 2):
        if pre is not None:
            x = rnd(pre, dt).double()
        t = rnd(conv_step(f"{name}/b{k}c1", x, ws[2 * k], bs[2 * k], relu=True), dt).double()
        pre = conv_step(f"{name}/b{k}c2", t, ws[2 * k + 1], bs[2 * k + 1], res=x, relu=True)
    return pre


def tower_case(B, nb, gather, fused=False, elem=0):
    name = f"tower-B{B}-nb{nb}-g{gather}" + (f"-fused-e{elem}" if fused else "")
    g = _gen(11, B, nb, gather, int(fused), elem)
    C, H, W, A = 256, 4, 5, 3
    S1 = 3 if gather else 1
    dt = FP16 if elem else BF16
    pool = ints(g, (B, S1, H, W, C), 0, 63 if elem else CHAIN_AMAX)
    slot = slots_for(B, S1)
    ws = [sparse_w(g, C, C, 3) for _ in range(2 * nb)]
    bs = [ints(g, (C,), -6, 0) for _ in range(2 * nb)]
    x = nchw(pool[torch.arange(B), slot.long()])
    c = dict(name=name, B=B, nb=nb, S1=S1, pool=pool, slot=slot, ws=ws, bs=bs, elem=elem, dims=("env", "y", "x", "channel"))
    if fused:
        c.update(w0=sparse_w(g, C, C, 3), b0=ints(g, (C,), -4, 0), tab=ints(g, (H * W, A, C), -2, 2), act=acts_for(B, A), A=A)
        x = rnd(conv_step(name + "/w0", x, c["w0"], c["b0"], extra=table_rows(c["tab"], c["act"], H, W), relu=True), dt).double()
    pre = res_chain(name, x, ws, bs, dt)
    if elem:
        assert float(pre.max()) < 2.0 ** 15, "fp16 image out of range"
    c["pre"], c["dt"] = pre, dt
    c["ref"] = nhwc(rnd(pre, dt).to(BF16))  # the fp16 image leaves as bf16 (towerp.hip's header)
    return c


# ------------------------------------------------------------------------------------------------ conv_lat
# (B, H, W, Cin, Cout, ks, gather, action bias, residual, relu). E = 160 / HW envs per workgroup (E3 = 96 / HW on the
# 3-row tiles): 4x5 -> 8 (4), 8x10 -> 2 (1), 3x7 -> 7 (4), 2x3 -> 26 (16). Cout 160: a partial second column block.
LAT_CASES = [(1, 4, 5, 256, 256, 3, 1, 1, 1, 1), (7, 4, 5, 256, 160, 3, 0, 0, 1, 0), (8, 4, 5, 128, 128, 1, 1, 1, 0, 1),
             (9, 4, 5, 64, 32, 3, 0, 1, 1, 1), (17, 4, 5, 256, 256, 1, 1, 0, 1, 1), (17, 4, 5, 128, 160, 3, 0, 1, 0, 0),
             (9, 4, 5, 64, 160, 1, 1, 0, 0, 0), (1, 8, 10, 256, 128, 3, 0, 0, 1, 1), (3, 8, 10, 128, 256, 3, 1, 1, 1, 0),
             (3, 8, 10, 64, 160, 1, 0, 0, 0, 1), (8, 3, 7, 256, 256, 3, 1, 1, 1, 1), (5, 2, 3, 128, 32, 1, 0, 1, 1, 0)]
LAT_BN_CASES = [(9, 4, 5, 256, 256, 3), (17, 4, 5, 128, 128, 1), (3, 8, 10, 128, 256, 3)]  # x modes 0, 1, 2
# the input-gradient use: (kind, H, W, Cin, Cout, ks) of the forward conv whose dx is taken
FLIP_CASES = [("lat", 4, 5, 256, 256, 3), ("lat", 4, 5, 256, 128, 1), ("lat", 8, 10, 128, 256, 3),
              ("band", 16, 20, 128, 256, 3), ("band", 16, 20, 256, 128, 3)]


def conv_case(tag, B, H, W, Cin, Cout, ks, gather, ab, res, relu, S1=3, A=3):
    """One dense-grid bf16 conv with the optional slot gather, action-bias table and residual."""
    name = f"{tag}-B{B}-{H}x{W}-{Cin}-{Cout}-k{ks}-g{gather}a{ab}r{res}u{relu}"
    g = _gen(sum(map(ord, tag)), B, H, W, Cin, Cout, ks, gather, ab, res, relu)
    S = S1 if gather else 1
    pool = ints(g, (B, S, H, W, Cin), 0 if gather else -3, 3)
    slot = slots_for(B, S)
    c = dict(name=name, B=B, H=H, W=W, Cin=Cin, Cout=Cout, ks=ks, S1=S, pool=pool, slot=slot, relu=relu,
             w=dense_w(g, Cout, Cin, ks), b=tie_bias(g, Cout), tab=None, act=None, res=None, A=A,
             dims=("env", "y", "x", "channel"))
    extra = None
    if ab:
        c["tab"], c["act"] = ints(g, (H * W, A, Cout), -4, 4), acts_for(B, A)
        extra = table_rows(c["tab"], c["act"], H, W)
    if res:
        c["res"] = ints(g, (B, H, W, Cout), -5, 5)
    x = nchw(pool[torch.arange(B), slot.long()])
    c["pre"] = conv_step(name, x, c["w"], c["b"], extra=extra, res=None if c["res"] is None else nchw(c["res"]), relu=bool(relu))
    c["ref"] = nhwc(rnd(c["pre"], BF16))
    return c


def lat_case(*p):
    return conv_case("lat", *p)


def lat_bn_case(B, H, W, Cin, Cout, ks):
    """mzba_conv_lat_bn's `out` in modes 0 (conv + bias + res), 1 (conv + bias) and 2 (bf16(conv + bias + res)
    [y > 0] with an integer y)."""
    c = conv_case("latbn", B, H, W, Cin, Cout, ks, 0, 0, 1, 0)
    g = _gen(13, B, H, W, Cin, Cout, ks)
    c["y"], c["xbn"] = ints(g, (B, H, W, Cout), -2, 2), ints(g, (B, H, W, Cout), -3, 3)
    x = nchw(c["pool"][:, 0])
    c["pre1"] = conv_step(c["name"] + "/m1", x, c["w"], c["b"])
    c["ref0"], c["ref1"] = c["ref"], nhwc(rnd(c["pre1"], BF16))
    c["ref2"] = torch.where(c["y"] > 0, c["ref"].double(), torch.zeros(())).to(BF16)
    return c


def flip_case(kind, H, W, Cin, Cout, ks):
    """dx of a conv with master weights w [Cout][taps][Cin] from dy [B][H][W][Cout]: torch.nn.grad.conv2d_input, which
    is the conv of dy with the flipped, transposed weights (the form the certificate is evaluated on)."""
    name = f"flip-{kind}-{H}x{W}-{Cin}-{Cout}-k{ks}"
    g = _gen(17, H, W, Cin, Cout, ks, len(kind))
    B = 3
    w = ints(g, (Cout, ks * ks, Cin), -2, 2)
    dy = ints(g, (B, H, W, Cout), -3, 3)
    b = tie_bias(g, Cin)
    w_oihw = w.view(Cout, ks, ks, Cin).permute(0, 3, 1, 2).contiguous()
    wt = w_oihw.flip(2, 3).transpose(0, 1).contiguous()
    pre = conv_step(name, nchw(dy), wt, b)
    gi = torch.nn.grad.conv2d_input((B, Cin, H, W), w_oihw, nchw(dy), padding=ks // 2) + b.view(1, -1, 1, 1)
    assert torch.equal(pre, gi), name
    return dict(name=name, kind=kind, B=B, H=H, W=W, Cin=Cin, Cout=Cout, ks=ks, w=w, dy=dy, b=b, wt=wt, pre=pre,
                ref=nhwc(rnd(pre, BF16)), dims=("env", "y", "x", "channel"))


# ------------------------------------------------------------------------------------------------ conv_halo
# (B, H, W, Cin, Cout, relu, residual): every (B, H, W) x Cin {128, 256} x Cout {128, 256, 512} that
# mzba_conv_halo_supported accepts. 441 pixels: a ragged last 256-pixel tile and tiles that straddle envs; W = 23 / 24:
# one staged 256-channel block / two; 84x84: the widest halo; (5, 2, 2): 20 pixels, less than one tile, supported as it
# stands. The support check refuses Cin 256 -> Cout 128 at W > 23 (Cout 128 needs the whole Cin in one staged block):
# at (2, 24, 24) and (1, 84, 84) the nearest supported shape, the same image at Cout 256, is in the product already.
HALO_SHAPES = [(1, 21, 21), (3, 21, 21), (2, 23, 23), (2, 24, 24), (1, 84, 84), (5, 2, 2)]
HALO_CASES = [(B, H, W, Cin, Cout) for B, H, W in HALO_SHAPES for Cin in (128, 256) for Cout in (128, 256, 512)
              if not (Cin == 256 and Cout == 128 and W > 23)]
HALO_CASES = [p + (int(i % 4 < 2), int(i % 5 != 0)) for i, p in enumerate(HALO_CASES)]
HALO_GATHER_CASES = [(3, 5), (9, 2)]  # (B, S): 21x21, 256 -> 256, S + 1 latents per env, A = 3


def halo_case(B, H, W, Cin, Cout, relu, res):
    return conv_case("halo", B, H, W, Cin, Cout, 3, 0, 0, res, relu)


def halo_gather_case(B, S):
    return conv_case("halog", B, 21, 21, 256, 256, 3, 1, 1, 0, 1, S1=S + 1)


# ------------------------------------------------------------------------------------------------ band family
# (B, Cin, Cout, residual, relu): every supported (Cin, Cout) of mzba_conv_band; each runs xt 5 and 10
BAND_CASES = [(1, 64, 128, 0, 0), (3, 128, 128, 1, 1), (1, 128, 256, 0, 1), (3, 256, 128, 1, 0), (3, 256, 256, 1, 1),
              (1, 256, 256, 0, 0)]
BAND_RES_CASES = [(1, 128), (3, 256)]                  # (B, C)
REP_BLOCKS_CASES = [(3, 1), (1, 2)]                    # (B, nblocks)
REP_TRUNK_CASES = [(1, 0, 1), (3, 1, 0), (1, 1, 1), (3, 0, 1)]  # (B, n0, n1)


def band_case(B, Cin, Cout, res, relu):
    return conv_case("band", B, 16, 20, Cin, Cout, 3, 0, 0, res, relu)


def chain_case(tag, B, shapes, plain):
    """A sparse-grid chain at 16x20. shapes: (Cin, Cout) per conv; plain: indices of convs that stand alone (no ReLU,
    no residual: the trunk's stem and widening conv); the others pair up into ResidualBlocks."""
    name = f"{tag}-B{B}-" + "-".join(str(co) for _, co in shapes)
    g = _gen(sum(map(ord, tag)), B, len(shapes), *[co for _, co in shapes])
    x = ints(g, (B, shapes[0][0], 16, 20), 0, CHAIN_AMAX)
    ws = [sparse_w(g, co, ci, 3) for ci, co in shapes]
    bs = [ints(g, (co,), -6, 0) for _, co in shapes]
    c = dict(name=name, B=B, x=nhwc(x), ws=ws, bs=bs, dims=("env", "y", "x", "channel"))
    cur, pre, k = x, None, 0
    while k < len(shapes):
        if pre is not None:
            cur = rnd(pre, BF16).double()
        if k in plain:
            pre, k = conv_step(f"{name}/c{k}", cur, ws[k], bs[k]), k + 1
        else:
            pre, k = res_chain(f"{name}/c{k}", cur, ws[k:k + 2], bs[k:k + 2], BF16), k + 2
            c["last_relu"] = pre  # the last activation a ReLU has shaped (the trunk may end on its widening conv)
    c["pre"], c["ref"] = pre, nhwc(rnd(pre, BF16))
    return c


def band_res_case(B, C):
    return chain_case("bandres", B, [(C, C)] * 2, ())


def rep_blocks_case(B, nb):
    return chain_case("repblocks", B, [(256, 256)] * (2 * nb), ())


def rep_trunk_case(B, n0, n1):
    shapes = [(64, 128)] + [(128, 128)] * (2 * n0) + [(128, 256)] + [(256, 256)] * (2 * n1)
    return chain_case("trunk", B, shapes, (0, 2 * n0 + 1))


# ------------------------------------------------------------------------------------------------ wgrad
# (B, H, W, Cin, Cout, ks, dtypes)
WGRAD_CASES = [(1, 4, 5, 256, 256, 3, ("f32", "bf16")), (9, 4, 5, 264, 256, 3, ("f32", "bf16")), (5, 4, 5, 40, 24, 3, ("f32",)),
               (3, 8, 10, 256, 256, 3, ("f32", "bf16")), (2, 16, 20, 64, 128, 3, ("f32", "bf16")),
               (7, 4, 5, 256, 128, 1, ("f32", "bf16"))]
# (nseg, B, H, W, Cin): Cout 256, bf16; variants 1 and 2, forms 0-3. The last: 5 x 512 envs, where variant 1 itself
# takes the whole-image kernel (wgrad.hip wgrad_img_eligible: nseg B >= 2048)
WGRAD_SEGS_CASES = [(1, 1, 4, 5, 256), (3, 7, 4, 5, 256), (2, 24, 3, 7, 256), (5, 33, 4, 5, 256), (1, 1, 4, 5, 264),
                    (3, 7, 4, 5, 264), (2, 24, 3, 7, 264), (5, 33, 4, 5, 264), (5, 512, 4, 5, 256)]


def wgrad_case(nseg, B, H, W, Cin, Cout, ks):
    """dw [Cout][taps][Cin] and db [Cout] accumulated onto integer dw0 / db0, over nseg segments of B envs. Every term is
    an integer; the certificate's sum of magnitudes is bounded by (pixels) max|x| max|dy| + |dw0| (an upper bound of the
    conv of the absolute values: the condition checked is stricter than the stated one)."""
    name = f"wgrad-s{nseg}-B{B}-{H}x{W}-{Cin}-{Cout}-k{ks}"
    g = _gen(19, nseg, B, H, W, Cin, Cout, ks)
    xs = [ints(g, (B, H, W, Cin), -3, 3) for _ in range(nseg)]
    dys = [ints(g, (B, H, W, Cout), -3, 3) for _ in range(nseg)]
    dw0, db0 = ints(g, (Cout, ks * ks, Cin), -9, 9), ints(g, (Cout,), -9, 9)
    x, dy = torch.cat(xs), torch.cat(dys)
    certify(name, torch.tensor(float(nseg * B * H * W) * float(x.abs().max()) * float(dy.abs().max()) + 9.0), 1.0)
    dw = torch.nn.grad.conv2d_weight(nchw(x), (Cout, Cin, ks, ks), nchw(dy), padding=ks // 2)
    dw = dw.permute(0, 2, 3, 1).reshape(Cout, ks * ks, Cin) + dw0
    db = dy.sum(dim=(0, 1, 2)) + db0
    return dict(name=name, nseg=nseg, B=B, H=H, W=W, Cin=Cin, Cout=Cout, ks=ks, xs=xs, dys=dys, dw0=dw0, db0=db0,
                dw=rnd(dw, F32), db=rnd(db, F32))


# ------------------------------------------------------------------------------------------------ f32 parity convs
# pixel-tiled forms at the 4x5 latent, Cin 256: (B, Cout, ks, mode), mode in plain / res / gather (+ action bias)
XT_CASES = [(1, 256, 3, "res"), (16, 128, 3, "gather"), (17, 256, 3, "gather"), (17, 256, 1, "res"), (16, 128, 1, "plain"),
            (1, 128, 3, "plain"), (17, 256, 3, "plain")]
# halo / pre-split forms: (B, H, W, Cin, Cout, relu, residual)
XP_CASES = [(1, 16, 20, 256, 256, 1, 1), (3, 16, 20, 128, 256, 0, 1), (3, 16, 20, 128, 128, 1, 0), (1, 8, 10, 256, 256, 0, 0),
            (3, 8, 10, 256, 256, 1, 1), (17, 4, 5, 256, 256, 1, 1)]
# two-part grid, one case per form: (form, which operand carries two parts)
X2_FORMS = ["x6t", "x6p", "x6r", "x3t", "x3p"]  # pixel-tiled, pre-split, per-read-split; x3 pixel-tiled, pre-split


def x_case(tag, B, H, W, Cin, Cout, ks, mode, relu, two=None):
    """An f32 conv. two = None: dense grid; "x": activations i + j 2^-12 with sparse integer weights; "w": two-part
    sparse weights with integer activations."""
    name = f"{tag}-B{B}-{H}x{W}-{Cin}-{Cout}-k{ks}-{mode}-u{relu}" + (f"-two{two}" if two else "")
    g = _gen(sum(map(ord, tag)), B, H, W, Cin, Cout, ks, len(mode), relu, 0 if two is None else ord(two))
    S1, A = (3, 3) if mode == "gather" else (1, 3)
    if two == "x":
        i = ints(g, (B, S1, H, W, Cin), 1, 3) * (ints(g, (B, S1, H, W, Cin), 0, 1) * 2 - 1)
        pool = i + (ints(g, (B, S1, H, W, Cin), 0, 1) * 2 - 1) * 2.0 ** -12
    else:
        pool = ints(g, (B, S1, H, W, Cin), -3, 3)
    w = dense_w(g, Cout, Cin, ks) if two is None else sparse_w(g, Cout, Cin, ks, two_part=two == "w")
    slot = slots_for(B, S1)
    c = dict(name=name, B=B, H=H, W=W, Cin=Cin, Cout=Cout, ks=ks, S1=S1, A=A, pool=pool, slot=slot, w=w, relu=relu,
             b=ints(g, (Cout,), -8, 8), tab=None, act=None, res=None, two=two, dims=("env", "y", "x", "channel"))
    extra = None
    if mode == "gather":
        c["tab"], c["act"] = ints(g, (H * W, A, Cout), -4, 4), acts_for(B, A)
        extra = table_rows(c["tab"], c["act"], H, W)
    if mode == "res":
        c["res"] = ints(g, (B, H, W, Cout), -5, 5)
    x = nchw(pool[torch.arange(B), slot.long()])
    c["pre"] = conv_step(name, x, w, c["b"], extra=extra, res=None if c["res"] is None else nchw(c["res"]), relu=bool(relu))
    c["ref"] = nhwc(rnd(c["pre"], F32))
    return c


def xt_case(B, Cout, ks, mode):
    return x_case("xt", B, 4, 5, 256, Cout, ks, mode, 0 if mode == "plain" else 1)


def xp_case(B, H, W, Cin, Cout, relu, res):
    return x_case("xp", B, H, W, Cin, Cout, 3, "res" if res else "plain", relu)


def x2_case(form, two):
    """The two-part case of one form: the pixel-tiled forms at 4x5 (B = 3), the halo forms at 8x10 (B = 1)."""
    if form in ("x6t", "x3t"):
        return x_case("x2" + form, 3, 4, 5, 256, 256, 3, "res", 1, two=two)
    return x_case("x2" + form, 1, 8, 10, 256, 256, 3, "res", 1, two=two)


# ------------------------------------------------------------------------------------------------ reporting
def _ranges(idx):
    idx = sorted(set(int(i) for i in idx))
    out, s, p = [], idx[0], idx[0]
    for i in idx[1:] + [None]:
        if i is None or i != p + 1:
            out.append(f"{s}" if s == p else f"{s}-{p}")
            s = i
        p = i
    return ",".join(out)


def assert_bits_equal(name, got, ref, dims):
    """got == ref as integers, element by element. On a mismatch: the count, the first 10 differing elements decoded
    along `dims` with got / want, and the differing set's extent per axis (the last axis also in 16-channel blocks), so
    the failing tile can be read off the log."""
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    assert len(dims) == got.dim(), (name, dims, got.shape)
    view = torch.int16 if got.element_size() == 2 else torch.int32
    bad = (got.view(view) != ref.view(view)).nonzero()
    if bad.shape[0] == 0:
        return
    lines = [f"{name}: {bad.shape[0]} of {got.numel()} elements differ"]
    for ix in bad[:10].tolist():
        where = ", ".join(f"{d} {i}" for d, i in zip(dims, ix))
        lines.append(f"  ({where}): got {float(got[tuple(ix)])!r} want {float(ref[tuple(ix)])!r}")
    for a, d in enumerate(dims):
        lines.append(f"  {d}: {_ranges(bad[:, a].tolist())}")
    lines.append(f"  {dims[-1]} blocks of 16: {_ranges((bad[:, -1] // 16).tolist())}")
    msg = "\n".join(lines)
    print(msg)
    raise AssertionError(msg)
