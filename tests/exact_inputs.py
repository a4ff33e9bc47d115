"""Inputs on which the bf16 products have ONE right answer, and the plain restatements that give it.

Every operand sits on a dyadic grid (integers, eighths) small enough that each x*w product and every partial sum of an output is an exact
fp32 number: the order of the sum, the split of the K loop, MFMA accumulation and split-row reductions cannot change the value, so a kernel
that computes in fp32 and rounds once must return the exact sum rounded once to nearest-even, bit for bit.  A dropped tap, truncation,
round-half-away, a second rounding or a bias taken through bf16 changes at least one bit (tests/test_exact_inputs_cpu.py shows that for every
case below); tests/test_exact_products_gpu.py holds the kernels to it.

A `Ref` is one output of one op: product(*operands) (+ bias) (+ residual) (ReLU) (post), in fp64 on whatever device the operands are on.
The `*_operands(case)` functions make the seeded fp64 operands of a case on the CPU, the `*_refs(o)` functions the Refs of every output and
epilogue variant the GPU test compares; both tests go through the same two functions.  Nothing here needs a GPU."""
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

BF16, F32 = torch.bfloat16, torch.float32
EXACT_UNITS = 2 ** 24          # fp32 holds every multiple of q below 2^24 q: sums of terms on the grid q stay exact under it, in any order

# ---- the cases (tests/test_exact_products_gpu.py runs them on the kernels, tests/test_exact_inputs_cpu.py proves what they can detect) ----
CONV_C64 = [(3, 64, 9, 11, 64), (2, 64, 30, 41, 64), (3, 64, 1, 1, 64), (2, 64, 9, 70, 64)]                                    # (n, c, h, w, k): kernel 4
CONV_TILE = [(1, 128, 7, 7, 256), (2, 192, 12, 12, 64), (5, 128, 16, 10, 48), (4, 64, 14, 14, 160), (33, 64, 2, 3, 128)]        # kernels 5 .. 11, 0
CONV_IGEMM = [(1, 32, 9, 11, 128, 5, 2, 2), (2, 64, 20, 80, 128, 3, 1, 1), (3, 128, 14, 14, 256, 1, 2, 0), (2, 64, 5, 4, 128, 1, 1, 0),
              (2, 64, 28, 28, 128, 3, 2, 1)]                                                                                     # (.., rs, stride, pad)
CONV_DOWN = [(2, 32, 9, 11, 128, 5, 2), (1, 64, 31, 17, 128, 3, 2)]                                                              # (n, c, h, w, k, rs, stride)
CONV_CAT = [(9, 64, 64, 7, 5, 48), (2, 192, 64, 10, 33, 160)]                                                                    # (n, c1, c2, h, w, k)
CONV_UPCAT = [(5, 3, 3, 128, 64, 128), (5, 3, 3, 64, 128, 64), (5, 4, 4, 256, 64, 64), (5, 4, 4, 64, 64, 128)]                   # (n, hl, wl, c1, c2, k)
STEM = [(1, 8, 8), (2, 30, 44), (1, 57, 23), (5, 2, 2)]                                                                          # (n, hs, ws)
STEM_NCHW = [(1, 2, 114, 46), (5, 3, 4, 4)]                                                                                      # (n, c, h, w)
TRAIN_CONV = [(3, 64, 192, 9, 13), (2, 384, 128, 14, 14), (2, 64, 64, 28, 28)]                                                   # (n, c, k, h, w)
TRAIN_WGRAD = TRAIN_CONV + [(5, 64, 64, 3, 2)]
TRAIN_S2 = [(2, 64, 128, 15, 13), (1, 128, 128, 7, 9), (5, 64, 256, 2, 2)]                                                       # (n, c, k, h, w)
WGRAD_STRIDED = [(3, 128, 40, 9, 9, 1, 2, 0), (1, 64, 72, 16, 16, 5, 2, 2)]                                                      # (n, c, k, h, w, r, stride, pad)
TRAIN_STEM = [(2, 1, 64, 48), (1, 4, 130, 118)]                                                                                  # (n, c, h, w)
GEMM = [(130, 40, 32), (1001, 64, 256), (1, 8, 64)]                                                                              # (M, N, K)
TOKEN_LINEAR = [(1001, 64, 40)]                                                                                                  # (rows, cin, cout)
PROJ_ROWS = [(77, 64, (16, 32)), (129, 32, (16, 16, 16)), (5, 512, (48,))]                                                       # (rows, k, widths)
HEAD = [(3, 32, 5, 7, 3), (1, 256, 3, 3, 8)]                                                                                     # (n, c, h, w, classes)
HEAD_BWD = [(2, 32, 9, 5, 4)]
BIAS_ACT = [(2, 8, 5, 7), (1, 256, 7, 7)]
POOL = [(3, 16, 9, 11), (2, 24, 4, 7)]


# ---- seeded operands on dyadic grids (fp64, CPU) ----
def generator(*key):
    """A CPU generator seeded by the case itself (any nesting of ints and strings)."""
    seed = 0
    for v in str(key).encode():
        seed = (seed * 1000003 + v) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def integers(g, *shape):
    """Activations, output gradients, residuals: integers in [-8, 8]."""
    return torch.randint(-8, 9, shape, generator=g).double()


def weights(g, *shape):
    """m / 8 with |m| <= 4: an fp32 master weight on this grid casts to bf16 exactly."""
    return torch.randint(-4, 5, shape, generator=g).double() / 8


def biases(g, n):
    """m / 8 with m odd and 2^8 < |m| < 2^10, for the ops whose contract keeps the bias in fp32: nine or ten significant bits, so NO value
    is a bf16 number and a bias taken through bf16 is a different bias."""
    m = 2 * torch.randint(128, 512, (n,), generator=g) + 1
    return (m * (2 * torch.randint(0, 2, (n,), generator=g) - 1)).double() / 8


def lowres(g, *shape):
    """Inputs of the 2x enlargement: multiples of 16, so every 1/4 - 3/4 blend (weights 9/16, 3/16, 3/16, 1/16) is an integer.  -16, 0, 16
    only: the enlarged values stay within [-16, 16], the convolution's sums within a few hundred, where bf16's spacing is 1 or 2 and one
    sum in eight is a tie; with inputs up to 128 the sums pass 1000 (spacing 4 to 8) and too few ties are left for the 2% floor."""
    return 16 * torch.randint(-1, 2, shape, generator=g).double()


def on(o, device):
    """The operands of a case on `device` (still fp64: the restatement runs there; the test casts what it hands to the kernel)."""
    return NS(**{k: v.to(device) if torch.is_tensor(v) else v for k, v in vars(o).items()})


# ---- the plain products (fp64, any device) ----
def conv(x, w, stride=1, pad=1):
    return F.conv2d(x, w, None, stride, pad)


def conv_dgrad(dy, w, shape=None, stride=1, pad=1):
    return torch.nn.grad.conv2d_input(shape, w, dy, stride, pad)


def conv_wgrad(x, dy, shape=None, stride=1, pad=1):
    return torch.nn.grad.conv2d_weight(x, shape, dy, stride, pad)


def s2_dgrad(dy, w, dyd, wd, shape=None):
    """The gradient of a strided block's input: the 3x3 / stride-2 / pad-1 branch and the 1x1 / stride-2 branch in one sum."""
    return conv_dgrad(dy, w, shape, 2, 1) + conv_dgrad(dyd, wd, shape, 2, 0)


def cat_conv(x1, x2, w):
    return conv(torch.cat([x1, x2], 1), w)


def enlarge2x(lo):
    """The exact 2x bilinear enlargement (align_corners = false): the weights are 1/4 and 3/4, exact in any float format."""
    return F.interpolate(lo, scale_factor=2, mode="bilinear", align_corners=False)


def upcat_conv(lo, x2, w):
    return cat_conv(enlarge2x(lo), x2, w)


def stem_s2d(x):
    """[N, C <= 4, H, W] -> the stem's space-to-depth image [N, 16, H/2, W/2]: channel (c*2+p)*2+q = x[c, 2i+p, 2j+q], zeros above 4C."""
    s = F.pixel_unshuffle(x, 2)
    return F.pad(s, (0, 0, 0, 0, 0, 16 - s.shape[1]))


def stem_conv4(xs, w):
    """The stem on the space-to-depth image: 4x4 window, pad 2, the top-left Hs x Ws outputs."""
    return F.conv2d(xs, w, None, 1, 2)[:, :, :xs.shape[2], :xs.shape[3]]


def stem_conv4_nchw(x, w):
    return stem_conv4(stem_s2d(x), w)


def nt(a, bt):
    return a @ bt.t()


def tn(dy, x):
    return dy.t() @ x


def column_sums(dy):
    return dy.sum(0)


def channel_sums(dz):
    return dz.sum((0, 2, 3))


def same(x):
    return x


def pool3x3s2(x):
    return F.max_pool2d(x, 3, 2, 1)


# ---- rounding ----
def round_once(ref64, dtype):
    """fp64 -> fp32 (which must be exact: the value is what an fp32 accumulator holds) -> bf16 by nearest-even; fp32 outputs stay fp32."""
    f32 = ref64.float()
    assert torch.equal(f32.double(), ref64), "the reference value is not an fp32 number: the inputs are not exactly summable"
    return f32 if dtype == F32 else f32.to(dtype)


def _bits(f32):
    return f32.contiguous().view(torch.int32)


def truncate_to_bf16(f32):
    """MUTANT: drop the low 16 bits."""
    return (_bits(f32) & -65536).view(F32).bfloat16()


def half_away_to_bf16(f32):
    """MUTANT: nearest, ties away from zero (sign-magnitude: adding half a unit to the bit pattern rounds the magnitude)."""
    return ((_bits(f32) + 0x8000) & -65536).view(F32).bfloat16()


def rounding_stats(ref64):
    """(fraction of values that are no bf16 number, fraction that are ties nearest-even rounds DOWN -- where half-away differs)."""
    b = _bits(ref64.float())
    low = b & 0xFFFF
    ties_down = (low == 0x8000) & ((b >> 16) & 1 == 0)
    return (low != 0).double().mean().item(), ties_down.double().mean().item()


# ---- one output of one op ----
class Ref:
    """post(relu(product(*operands, **kw) + bias + residual)) in fp64; `bias` / `residual` already broadcast against the product.
    dtype: the type the kernel returns it in.  quantum: the grid every term (each product, the bias, the residual) lies on."""

    def __init__(self, product, *operands, bias=None, residual=None, relu=False, post=None, dtype=BF16, quantum=1 / 8, _shared=None, **kw):
        self.product, self.operands, self.kw = product, operands, kw
        self.bias, self.residual, self.relu, self.post, self.dtype, self.quantum = bias, residual, relu, post, dtype, quantum
        self._shared = {} if _shared is None else _shared       # what the epilogue variants of one product have in common

    def variant(self, **changes):
        cur = dict(bias=self.bias, residual=self.residual, relu=self.relu, post=self.post, dtype=self.dtype, quantum=self.quantum)
        return Ref(self.product, *self.operands, **{**cur, **changes}, _shared=self._shared, **self.kw)

    def _cached(self, name, make):
        if name not in self._shared:
            self._shared[name] = make()
        return self._shared[name]

    @property
    def acc(self):
        return self._cached("acc", lambda: self.product(*self.operands, **self.kw))

    def value(self, acc=None, bias=None, round_before_residual=False):
        v = self.acc if acc is None else acc
        bias = self.bias if bias is None else bias
        if bias is not None:
            v = v + bias
        if round_before_residual:
            v = v.float().bfloat16().double()
        if self.residual is not None:
            v = v + self.residual
        if self.relu:
            v = v.relu()
        return v if self.post is None else self.post(v)

    @property
    def ref64(self):
        return self.value()

    def exact(self):
        """The one right answer in the kernel's output type."""
        return round_once(self.ref64, self.dtype)

    @property
    def mag64(self):
        """The sum of the absolute terms of every output: the product of the absolute operands + |bias| + |residual|."""
        m = self._cached("mag", lambda: self.product(*(t.abs() for t in self.operands), **self.kw))
        for t in (self.bias, self.residual):
            if t is not None:
                m = m + t.abs()
        return m

    @property
    def products(self):
        """The largest number of products summed into one output (taps that fall into the zero padding do not count)."""
        return int(self._cached("count", lambda: self.product(*(torch.ones_like(t) for t in self.operands), **self.kw).max().item()))

    # -- what a subtly wrong kernel would return (CPU test only) --
    def one_tap_dropped(self, smallest=False):
        """fp64 value with ONE element of the last operand (the weight) set to zero: the first non-zero one (smallest: the first of the
        smallest magnitude the operand has) that is live in this output -- a tap whose every product meets a zero input, or lands only in
        outputs the ReLU clamps or the pool discards, changes nothing a test could see."""
        last = self.operands[-1].reshape(-1)
        cand = torch.nonzero(last != 0 if not smallest else last.abs() == last.abs()[last != 0].min()).reshape(-1)
        if not smallest:                                    # spread over the operand (the output channels and window positions of a weight)
            cand = cand[torch.randperm(len(cand), generator=torch.Generator().manual_seed(len(cand))).to(cand.device)]
        for i in cand[:256].tolist():
            def drop():
                hit = last.clone()
                hit[i] = 0
                return self.product(*self.operands[:-1], hit.view(self.operands[-1].shape), **self.kw)
            v = self.value(acc=self._cached(("tap", i), drop))
            if not torch.equal(v, self.ref64):
                return v
        raise AssertionError("no live tap among 256 candidates")

    def mutants(self):
        out = {"one tap dropped": round_once(self.one_tap_dropped(), self.dtype)}
        if self.dtype == BF16:
            f32 = self.ref64.float()
            out["truncation"] = truncate_to_bf16(f32)
            out["round-half-away"] = half_away_to_bf16(f32)
            if self.residual is not None:
                out["rounded before the residual"] = self.value(round_before_residual=True).float().bfloat16()
        if self.bias is not None:
            out["bias through bf16"] = round_once(self.value(bias=self.bias.float().bfloat16().double()), self.dtype)
        return out


def assert_exactly_summable(ref):
    """The sufficient condition for every summation order to be exact in fp32: every term of every output of `ref` lies on the grid
    ref.quantum, and the sum of the ABSOLUTE terms of each output -- conv(|x|, |w|) + |bias| + |residual|, and likewise for the GEMMs, the
    data and the weight gradients -- is below 2^24 in units of that grid (the last bit any partial sum can need)."""
    q = ref.quantum
    for name, t in [("bias", ref.bias), ("residual", ref.residual), ("exact sum", ref.acc), ("sum of absolute terms", ref.mag64)]:
        if t is not None:
            u = t / q
            assert torch.equal(u, u.round()), f"{name} is not on the grid {q}"
    units = ref.mag64.max().item() / q
    assert units < EXACT_UNITS, f"sum of absolute terms {units:.0f} units of {q} >= 2^24: a partial sum could round"
    return units


def assert_bits(got, want):
    """torch.equal, and on failure how many elements differ, the first few with both values, and the largest difference in units of the
    last bit of `want` (bf16 units for a bf16 output)."""
    assert got.shape == want.shape and got.dtype == want.dtype, f"got {tuple(got.shape)} {got.dtype}, want {tuple(want.shape)} {want.dtype}"
    if torch.equal(got, want):
        return
    g, w = got.double(), want.double()
    bad = torch.nonzero(g != w)
    mant = 8 if want.dtype == BF16 else 24
    ulp = torch.exp2(torch.floor(torch.log2(w.abs().clamp_min(2.0 ** -126))) - (mant - 1))
    worst = ((g - w).abs() / ulp).max().item()
    first = "; ".join(f"{tuple(i.tolist())}: got {g[tuple(i)].item()!r} want {w[tuple(i)].item()!r}" for i in bad[:8])
    raise AssertionError(f"{len(bad)} of {w.numel()} elements differ (largest difference {worst:.3g} units of the last bit); first: {first}")


# ---- operands and Refs of every family of cases ----
def _b4(b):
    return b.view(1, -1, 1, 1)


def _epilogues(base, bias, residual):
    """{(relu, with residual): Ref}: the four epilogues of an inference convolution."""
    return {(relu, res): base.variant(bias=bias, residual=residual if res else None, relu=relu) for relu in (True, False) for res in (False, True)}


def conv_operands(case):
    n, c, h, w, k, rs, stride, pad = case if len(case) == 8 else (*case, 3, 1, 1)
    g = generator("conv", case)
    ho, wo = (h + 2 * pad - rs) // stride + 1, (w + 2 * pad - rs) // stride + 1
    return NS(x=integers(g, n, c, h, w), w=weights(g, k, c, rs, rs), b=biases(g, k), r=integers(g, n, k, ho, wo), stride=stride, pad=pad)


def conv_refs(o):
    return _epilogues(Ref(conv, o.x, o.w, stride=o.stride, pad=o.pad), _b4(o.b), o.r)


def down_operands(case):
    n, c, h, w, k, rs, stride = case
    g = generator("down", case)
    return NS(x=integers(g, n, c, h, w), w=weights(g, k, c, rs, rs), wd=weights(g, k, c, 1, 1), b=biases(g, k), bd=biases(g, k), stride=stride, pad=rs // 2)


def down_refs(o):
    """{("y", relu): .., ("yd", with branch bias): ..}"""
    y = Ref(conv, o.x, o.w, stride=o.stride, pad=o.pad, bias=_b4(o.b))
    yd = Ref(conv, o.x, o.wd, stride=o.stride, pad=0)
    return {("y", True): y.variant(relu=True), ("y", False): y, ("yd", False): yd, ("yd", True): yd.variant(bias=_b4(o.bd))}


def cat_operands(case):
    n, c1, c2, h, w, k = case
    g = generator("cat", case)
    return NS(x1=integers(g, n, c1, h, w), x2=integers(g, n, c2, h, w), w=weights(g, k, c1 + c2, 3, 3), b=biases(g, k), r=integers(g, n, k, h, w))


def cat_refs(o):
    return _epilogues(Ref(cat_conv, o.x1, o.x2, o.w), _b4(o.b), o.r)


def upcat_operands(case):
    n, hl, wl, c1, c2, k = case
    g = generator("upcat", case)
    return NS(lo=lowres(g, n, c1, hl, wl), x2=integers(g, n, c2, 2 * hl, 2 * wl), w=weights(g, k, c1 + c2, 3, 3), b=biases(g, k),
              r=integers(g, n, k, 2 * hl, 2 * wl))


def upcat_refs(o):
    """The four epilogues of the fused convolution, and "up": the enlargement alone (integers of at most 128: bf16 numbers, so the
    kernel's rounding of the enlarged feature to bf16 changes nothing)."""
    refs = _epilogues(Ref(upcat_conv, o.lo, o.x2, o.w), _b4(o.b), o.r)
    refs["up"] = Ref(enlarge2x, o.lo, quantum=1)
    return refs


def stem_operands(case):
    n, hs, ws = case
    g = generator("stem", case)
    return NS(xs=integers(g, n, 16, hs, ws), w=weights(g, 64, 16, 4, 4), b=biases(g, 64))


def stem_refs(o):
    return {"y": Ref(stem_conv4, o.xs, o.w, bias=_b4(o.b), relu=True, post=pool3x3s2)}


def stem_nchw_operands(case):
    n, c, h, w = case
    g = generator("stem_nchw", case)
    return NS(x=integers(g, n, c, h, w), w=weights(g, 64, 16, 4, 4), b=biases(g, 64))


def stem_nchw_refs(o):
    return {"y": Ref(stem_conv4_nchw, o.x, o.w, bias=_b4(o.b), relu=True, post=pool3x3s2)}


def train_conv_operands(case):
    n, c, k, h, w = case
    g = generator("train_conv", case)
    return NS(x=integers(g, n, c, h, w), w=weights(g, k, c, 3, 3), dy=integers(g, n, k, h, w))


def train_conv_refs(o):
    return {"y": Ref(conv, o.x, o.w), "dx": Ref(conv_dgrad, o.dy, o.w, shape=o.x.shape),
            "dw": Ref(conv_wgrad, o.x, o.dy, shape=o.w.shape, dtype=F32, quantum=1)}


def train_s2_operands(case):
    n, c, k, h, w = case
    g = generator("train_s2", case)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return NS(x=integers(g, n, c, h, w), w=weights(g, k, c, 3, 3), wd=weights(g, k, c, 1, 1), gy=integers(g, n, k, ho, wo), gyd=integers(g, n, k, ho, wo))


def train_s2_refs(o):
    return {"y": Ref(conv, o.x, o.w, stride=2, pad=1), "yd": Ref(conv, o.x, o.wd, stride=2, pad=0),
            "dx": Ref(s2_dgrad, o.gy, o.w, o.gyd, o.wd, shape=o.x.shape),
            "dw": Ref(conv_wgrad, o.x, o.gy, shape=o.w.shape, stride=2, pad=1, dtype=F32, quantum=1),
            "dwd": Ref(conv_wgrad, o.x, o.gyd, shape=o.wd.shape, stride=2, pad=0, dtype=F32, quantum=1)}


def wgrad_strided_operands(case):
    n, c, k, h, w, r, stride, pad = case
    g = generator("wgrad_strided", case)
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
    return NS(x=integers(g, n, c, h, w), dy=integers(g, n, k, ho, wo), wshape=(k, c, r, r), stride=stride, pad=pad)


def wgrad_strided_refs(o):
    return {"dw": Ref(conv_wgrad, o.x, o.dy, shape=o.wshape, stride=o.stride, pad=o.pad, dtype=F32, quantum=1)}


def train_stem_operands(case):
    n, c, h, w = case
    g = generator("train_stem", case)
    return NS(x=integers(g, n, c, h, w), w=weights(g, 64, c, 7, 7), gy=integers(g, n, 64, h // 2, w // 2))


def train_stem_refs(o):
    return {"y": Ref(conv, o.x, o.w, stride=2, pad=3), "dw": Ref(conv_wgrad, o.x, o.gy, shape=o.w.shape, stride=2, pad=3, dtype=F32, quantum=1)}


def gemm_operands(case):
    M, N, K = case
    g = generator("gemm", case)
    return NS(a=integers(g, M, K), bt=weights(g, N, K), bias=biases(g, N), b2=integers(g, M, N))


def gemm_refs(o):
    """C = a bt^T + bias in either type; the token-major weight gradient a^T b2 [K, N] and the column sums of a (fp32 whatever the inputs)."""
    c = Ref(nt, o.a, o.bt, bias=o.bias)
    return {("c", BF16): c, ("c", F32): c.variant(dtype=F32), "d": Ref(tn, o.a, o.b2, dtype=F32, quantum=1),
            "colsum": Ref(column_sums, o.a, dtype=F32, quantum=1)}


def token_linear_operands(case):
    rows, cin, cout = case
    g = generator("token_linear", case)
    return NS(x=integers(g, rows, cin), w=weights(g, cout, cin), b=biases(g, cout), dy=integers(g, rows, cout))


def token_linear_refs(o):
    """y = x W^T + b, dx = dy W in x's type; dW = dy^T x and db in fp32.  The op casts the weight to x's type (exact on this grid) and hands
    the bias to the product's epilogue as fp32 (ops._TokenLinear, gemm.hip: `acc += p.bias[..]` on the fp32 accumulator): no rounding of an
    operand to restate."""
    y, dx = Ref(nt, o.x, o.w, bias=o.b), Ref(nt, o.dy, o.w.t().contiguous())
    return {("y", BF16): y, ("y", F32): y.variant(dtype=F32), ("dx", BF16): dx, ("dx", F32): dx.variant(dtype=F32),
            "dw": Ref(tn, o.dy, o.x, dtype=F32, quantum=1), "db": Ref(column_sums, o.dy, dtype=F32, quantum=1)}


def proj_rows_operands(case):
    rows, k, widths = case
    g = generator("proj_rows", case)
    return NS(x=integers(g, rows, k), w=weights(g, sum(widths), k), b=biases(g, sum(widths)), widths=widths)


def proj_rows_refs(o):
    return {"out": Ref(nt, o.x, o.w, bias=o.b)}            # (the projections side by side: the test cuts the columns)


def head_operands(case):
    n, c, h, w, ncls = case
    g = generator("head", case)
    return NS(x=integers(g, n, c, h, w), w=weights(g, ncls, c, 1, 1), b=biases(g, ncls), gz=integers(g, n, ncls, h, w))


def head_refs(o):
    z = Ref(conv, o.x, o.w, stride=1, pad=0, bias=_b4(o.b))
    dx = Ref(conv_dgrad, o.gz, o.w, shape=o.x.shape, stride=1, pad=0)
    return {("z", BF16): z, ("z", F32): z.variant(dtype=F32), ("dx", BF16): dx, ("dx", F32): dx.variant(dtype=F32),
            "dw": Ref(conv_wgrad, o.x, o.gz, shape=o.w.shape, stride=1, pad=0, dtype=F32, quantum=1),
            "db": Ref(channel_sums, o.gz, dtype=F32, quantum=1)}


def bias_act_operands(shape):
    g = generator("bias_act", shape)
    return NS(x=integers(g, *shape), r=integers(g, *shape), b=biases(g, shape[1]))


def bias_act_refs(o):
    """{(dtype, relu, with residual): ..}"""
    base = Ref(same, o.x)
    return {(dt, *key): ref.variant(dtype=dt) for key, ref in _epilogues(base, _b4(o.b), o.r).items() for dt in (BF16, F32)}


def pool_operands(shape):
    g = generator("pool", shape)
    return NS(x=integers(g, *shape), b=biases(g, shape[1]))


def pool_refs(o):
    base = Ref(same, o.x, bias=_b4(o.b), relu=True, post=pool3x3s2)
    return {BF16: base, F32: base.variant(dtype=F32)}


# (name, cases, operands, refs): everything tests/test_exact_products_gpu.py runs, for tests/test_exact_inputs_cpu.py to go through
FAMILIES = [
    ("conv_bias_act kernel 4", CONV_C64, conv_operands, conv_refs),
    ("conv_bias_act kernels 5-11, 0", CONV_TILE, conv_operands, conv_refs),
    ("conv_bias_act kernel 9", CONV_IGEMM, conv_operands, conv_refs),
    ("conv_down_bias_act", CONV_DOWN, down_operands, down_refs),
    ("conv_cat_bias_act", CONV_CAT, cat_operands, cat_refs),
    ("conv_upcat_bias_act", CONV_UPCAT, upcat_operands, upcat_refs),
    ("stem_conv_pool", STEM, stem_operands, stem_refs),
    ("stem_conv_pool_nchw", STEM_NCHW, stem_nchw_operands, stem_nchw_refs),
    ("ops.conv3x3", TRAIN_WGRAD, train_conv_operands, train_conv_refs),
    ("ops.conv_s2_block", TRAIN_S2, train_s2_operands, train_s2_refs),
    ("ops.conv_wgrad_strided", WGRAD_STRIDED, wgrad_strided_operands, wgrad_strided_refs),
    ("ops.stem_conv", TRAIN_STEM, train_stem_operands, train_stem_refs),
    ("gemm_nt / wgrad", GEMM, gemm_operands, gemm_refs),
    ("token_linear", TOKEN_LINEAR, token_linear_operands, token_linear_refs),
    ("proj_rows", PROJ_ROWS, proj_rows_operands, proj_rows_refs),
    ("head_logits", HEAD, head_operands, head_refs),
    ("ops.head", HEAD_BWD, head_operands, head_refs),
    ("bias_act_", BIAS_ACT, bias_act_operands, bias_act_refs),
    ("bias_relu_maxpool", POOL, pool_operands, pool_refs),
]
