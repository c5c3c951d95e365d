"""Case tables, operands, float64 references, checks and test bodies for the GEMM family in every dispatch form
(tests/test_gpu_gemm_forms.py; the plans are asserted without a GPU by tests/test_gemm_dispatch.py; the bodies are re-run on the twin by
tests/test_cpu_twin.py and under poison by tests/test_gpu_unwritten.py and tests/test_poison_twin.py).  Pure Python: nothing here is a
test by itself.  The bodies call lib.sg_gemm / sg_gemm_nt* / sg_rowsum* / sg_segsum / sg_colsum directly on OPS.DEV.

Operands.  Every operand and every output is a view inside a larger buffer: a leading dimension larger than the extent and a non-zero
element offset (multiples of 4 where the case is a gemm128 / persistent case, not multiples of 4 where a skeleton case would otherwise
qualify for gemm128).  Operand buffers are NaN everywhere outside the view — more than a 32-k stage of padding columns behind every
row, four whole rows behind the last one, the elements before and after — so a kernel that sums anything outside its operands returns NaN.  Output buffers hold SENTINEL outside the written window and the
workspace is carved out of a larger buffer at exactly the byte count handed to the call, poisoned inside, fenced outside.

Checks per case.
 (a) exact: operands and biases are integers in [-4, 4], the epilogue is none, ReLU or LeakyReLU(0.5): every partial sum is an
     integer below 2^24 (|sum| <= 16 K + 8 with K <= 65 536 here), so every summation order is exact in fp32 and the result must be
     torch.equal to the float64 product.
 (b) rounded: randn operands, and a variant whose rows of A span 2^-20 .. 2^20.  Elementwise against a.double() @ b.double() + biases:
         |got - ref| <= 1.01 (K + S + 4) 2^-24 (|A| |B| + |bias_i| + |bias_j|)_ij
     the standard bound of a K-term fp32 dot product in any order plus S partial additions (S: the split count the plan query
     reports) and the epilogue's additions; LeakyReLU / ReLU are 1-Lipschitz and keep it; tanh / sigmoid add the atol = 1e-6 that
     test_activations grants sg_apply_act.  Nothing in it is measured.  Every check prints `[gemm-forms] case | variant | max |got -
     ref| / bound` before it asserts.
 (c) everything outside the output window still equals SENTINEL, the bytes around the workspace are untouched.
 (d) the output holds no NaN: the poisoned surroundings were never summed.
"""
import ctypes

import torch

import test_gpu_ops as OPS
from shapegan_amd import abi

SENTINEL = -777.25
FENCE = 0xA5
WS_CAP = 256 << 20                    # the workspace ops.gemm_raw passes: min(128 M N 4, 256 MiB)
EPS = 2.0 ** -24
ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
SKELETON, GEMM128, GEMM128_SPLIT, PERSISTENT = (abi.DEFINES["SG_GEMM_KIND_" + k] for k in ("SKELETON", "GEMM128", "GEMM128_SPLIT", "PERSISTENT"))
FIN_NONE, FIN_FLAT, FIN_DEEP = (abi.DEFINES["SG_GEMM_FINALIZE_" + k] for k in ("NONE", "FLAT", "DEEP"))
KIND_NAMES = {SKELETON: "skeleton", GEMM128: "gemm128", GEMM128_SPLIT: "gemm128-split", PERSISTENT: "persistent"}
SG_ERR_WORKSPACE = -3


def _lib():
    from shapegan_amd import ops
    return ops._lib()


def _seed(name):
    torch.manual_seed(sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31))


# ---- buffers -------------------------------------------------------------------------------------------------------------------------
def _ld(extent, aligned):
    """A leading dimension beyond `extent`: a multiple of 4 for the gemm128 family, not one otherwise."""
    if aligned:
        return (extent + 3) // 4 * 4 + 36                 # (more than a 32-k stage of NaN behind every row)
    ld = extent + 33
    return ld if ld % 4 else ld + 1


def embed(mat, ld, off, tail=None):
    """mat [R, C] as rows of stride ld inside a NaN buffer, starting at element `off` and followed by four whole NaN rows (the rows
    beyond M or N) and a few elements; returns the buffer on OPS.DEV."""
    R, C = mat.shape
    assert ld >= C
    tail = 4 * ld + 37 if tail is None else tail
    buf = torch.full((off + R * ld + tail,), float("nan"), dtype=torch.float32)
    buf[off:off + R * ld].view(R, ld)[:, :C] = mat
    return buf.to(OPS.DEV)


def embed_vec(v, off=3, tail=5):
    buf = torch.full((off + v.numel() + tail,), float("nan"), dtype=torch.float32)
    buf[off:off + v.numel()] = v
    return buf.to(OPS.DEV)


class Workspace(object):
    """`nbytes` poisoned bytes (0xFF: NaN as floats) between two fences of FENCE bytes; nbytes None: a null workspace."""
    PAD = 256

    def __init__(self, nbytes):
        self.nbytes = nbytes
        if nbytes is None:
            self.buf = None
            return
        self.buf = torch.full((nbytes + 2 * self.PAD,), FENCE, dtype=torch.uint8, device=OPS.DEV)
        self.poison()

    def poison(self):
        if self.buf is not None:
            self.buf[self.PAD:self.PAD + self.nbytes] = 0xFF

    def ptr(self):
        from shapegan_amd.lib import ptr
        return None if self.buf is None else ptr(self.buf) + self.PAD

    def address(self):
        return None if self.buf is None else self.buf.data_ptr() + self.PAD

    def check(self, what):
        if self.buf is not None:
            fences = torch.cat([self.buf[:self.PAD], self.buf[self.PAD + self.nbytes:]])
            assert bool((fences == FENCE).all()), what + ": a byte next to the workspace was written"


def take_window(buf, off, M, N, sci, scj, what):
    """The [M, N] window of an output buffer (a copy); asserts that every other element still is SENTINEL."""
    view = buf.as_strided((M, N), (sci, scj), off)
    got = view.clone()
    view.fill_(SENTINEL)
    assert bool((buf == SENTINEL).all()), what + ": an element outside the output window was written"
    return got.cpu()


# ---- sg_gemm cases --------------------------------------------------------------------------------------------------------------------
class Gemm(object):
    """One sg_gemm call.  la / lb: 'k' = k-major (A: element (i, k) at a[i * lda + k]; B: element (k, j) at b[j * ldb + k]), 'r' =
    row-major (a[k * lda + i]; b[k * ldb + j]).  aligned: leading dimensions and offsets that keep the 16-byte alignment gemm128
    needs.  ws: 'std' (what ops.gemm_raw passes), None (a null pointer), or a number of bytes.  c: 'row' (sci = N + 5 behind a column
    offset, scj = 1), 'transposed' (sci = 1, scj = M + 3), 'interleaved' (sci = 2, scj = 2 M + 2: sci < N without overlap).
    plan = (kind, tm, tn, nsplit, finalize): what the case claims to reach; tests/test_gemm_dispatch.py holds the launcher to it."""

    def __init__(self, la, lb, M, N, K, plan, aligned=None, ws="std", bias_i=False, bias_j=True, shift=0, act=ACT_NONE, c="row",
                 tag=""):
        self.la, self.lb, self.M, self.N, self.K, self.plan = la, lb, M, N, K, tuple(plan)
        self.aligned = plan[0] != SKELETON if aligned is None else aligned
        self.ws, self.bias_i, self.bias_j, self.shift, self.act, self.c = ws, bias_i, bias_j, shift, act, c
        self.slope = 0.5
        self.id = "%s-%s%s-%dx%dx%d%s" % (KIND_NAMES[plan[0]], la, lb, M, N, K, "-" + tag if tag else "")

    # layout of the call
    def ws_bytes(self):
        return min(128 * self.M * self.N * 4, WS_CAP) if self.ws == "std" else self.ws

    def strides(self):
        M, N, K = self.M, self.N, self.K
        lda = _ld(K if self.la == "k" else M, self.aligned)
        ldb = _ld(K if self.lb == "k" else N, self.aligned)
        sai, sak = (lda, 1) if self.la == "k" else (1, lda)
        sbk, sbj = (1, ldb) if self.lb == "k" else (ldb, 1)
        sci, scj = {"row": (N + 5, 1), "transposed": (1, M + 3), "interleaved": (2, 2 * M + 2)}[self.c]
        return lda, ldb, sai, sak, sbk, sbj, sci, scj

    def offsets(self):
        """element offsets of A, B and C inside their buffers"""
        return (8, 12, 3) if self.aligned else (3, 5, 3)

    def query(self, a_addr=None, b_addr=None, ws_addr="std"):
        """The plan the launcher itself launches from (host code).  Without addresses: the alignment the buffers of run() have."""
        _, _, sai, sak, sbk, sbj, sci, scj = self.strides()
        oa, ob, _ = self.offsets()
        a_addr = 0x10000 + 4 * oa if a_addr is None else a_addr
        b_addr = 0x20000 + 4 * ob if b_addr is None else b_addr
        nbytes = self.ws_bytes()
        if ws_addr == "std":
            ws_addr = None if nbytes is None else 0x30000
        return query_plan(a_addr, sai, sak, b_addr, sbk, sbj, sci, scj, self.bias_i, self.M, self.N, self.K, ws_addr, nbytes or 0)


def query_plan(a_addr, sai, sak, b_addr, sbk, sbj, sci, scj, bias_i, M, N, K, ws_addr, ws_bytes):
    from shapegan_amd import lib as L
    plan = (ctypes.c_long * 8)()
    L.check(L.load().sg_gemm_plan(a_addr, sai, sak, b_addr, sbk, sbj, sci, scj, int(bool(bias_i)), M, N, K, ws_addr, ws_bytes, plan), "gemm_plan")
    return {"kind": plan[0], "tm": plan[1], "tn": plan[2], "nsplit": plan[3], "kchunk": plan[4], "finalize": plan[5], "grid": plan[6],
            "layout": plan[7], "key": (plan[0], plan[1], plan[2], plan[3], plan[5])}


def query_nt_plan(batch, M, N, K):
    from shapegan_amd import lib as L
    plan = (ctypes.c_long * 5)()
    L.check(L.load().sg_gemm_nt_plan(batch, M, N, K, plan), "gemm_nt_plan")
    return {"direct": bool(plan[0]), "nsplit": plan[1], "kchunk": plan[2], "grid": plan[3], "ws_bytes": plan[4]}


LAYOUTS4 = [("k", "k"), ("k", "r"), ("r", "k"), ("r", "r")]
LAYOUTS3 = [("k", "k"), ("k", "r"), ("r", "r")]          # the gemm128 family has no row-major A x k-major B


def _skeleton_cases():
    out = []

    def add(M, N, K, tm, tn, S, fin, layouts=LAYOUTS4, **kw):
        for la, lb in layouts:
            out.append(Gemm(la, lb, M, N, K, (SKELETON, tm, tn, S, fin), **kw))

    for K in (3, 16, 17, 40):                             # one, two and three k-tiles with a tail
        add(5, 7, K, 1, 1, 1, FIN_NONE)
    add(1, 64, 256, 1, 1, 2, FIN_FLAT)                    # flat finalize, float4 loop / N % 4 != 0 loop
    add(1, 1, 256, 1, 1, 2, FIN_FLAT)
    add(1, 64, 4096, 1, 1, 32, FIN_DEEP)
    add(1, 1, 4096, 1, 1, 32, FIN_DEEP)
    add(4, 65537, 3, 1, 2, 1, FIN_NONE)                   # (513 column tiles of 128)
    add(1, 4100, 2050, 1, 2, 16, FIN_FLAT)
    add(1, 500, 16384, 1, 2, 128, FIN_DEEP)
    add(65, 129, 16384, 1, 2, 128, FIN_DEEP)
    add(2000, 2000, 3, 2, 1, 1, FIN_NONE)
    add(2000, 2000, 40, 2, 1, 1, FIN_NONE)
    add(4100, 1, 2050, 2, 1, 16, FIN_FLAT)
    add(500, 1, 16384, 2, 1, 128, FIN_DEEP)
    add(129, 100, 16384, 2, 1, 128, FIN_DEEP)
    add(2000, 4100, 3, 2, 2, 1, FIN_NONE)
    add(2000, 4100, 40, 2, 2, 1, FIN_NONE)
    add(129, 2000, 2050, 2, 2, 16, FIN_FLAT)
    add(2000, 129, 2050, 2, 2, 16, FIN_FLAT)
    add(129, 200, 16384, 2, 2, 128, FIN_DEEP)
    add(129, 129, 16384, 2, 2, 128, FIN_DEEP)
    # split counts through a capped workspace: the flat finalize's groups of four partials plus remainders of 1, 2 and 3
    for S in (3, 4, 5, 6, 7):
        add(1, 64, 4096, 1, 1, S, FIN_FLAT, ws=S * 64 * 4, tag="ws%d" % S)
    add(3, 64, 4096, 1, 1, 1, FIN_NONE, ws=None, tag="wsnull")
    # the epilogue's addressing and activations on the skeleton (one layout each; small enough for the twin)
    epi = [dict(bias_i=True, tag="biasi"), dict(c="transposed", tag="ct"), dict(c="interleaved", bias_i=True, tag="ci"),
           dict(shift=2, tag="shift2"), dict(act=ACT_LEAKY, tag="leaky"), dict(act=ACT_RELU, tag="relu"), dict(act=ACT_TANH, tag="tanh"),
           dict(act=ACT_SIGMOID, tag="sigmoid"), dict(bias_j=False, tag="nobias")]
    for n, kw in enumerate(epi):
        add(70, 130, 40, 1, 1, 1, FIN_NONE, layouts=[LAYOUTS4[n % 4]], **kw)
        add(3, 64, 4096, 1, 1, 32, FIN_DEEP, layouts=[LAYOUTS4[(n + 1) % 4]], **kw)
        add(3, 68, 256, 1, 1, 2, FIN_FLAT, layouts=[LAYOUTS4[(n + 2) % 4]], **kw)
    return out


def _gemm128_cases():
    out = []

    def add(M, N, K, kind, S, fin, layouts=LAYOUTS3, rr_M=None, **kw):
        for la, lb in layouts:
            out.append(Gemm(la, lb, rr_M if (rr_M and la == "r") else M, N, K, (kind, 0, 0, S, fin), **kw))

    for K in (64, 65, 67, 68, 95, 96, 97, 100, 129):      # one stage with a tail ... five stages; <= 512 tiles
        add(1000, 2000, K, GEMM128, 1, FIN_NONE)
    for K in (68, 129):                                   # more than 512 tiles, odd stage count: not persistent
        add(2000, 4100, K, GEMM128, 1, FIN_NONE)
    # more than 512 tiles, even stage count, persistent form refused by the epilogue
    add(2000, 4100, 64, GEMM128, 1, FIN_NONE, bias_i=True, tag="biasi")
    add(2000, 4100, 64, GEMM128, 1, FIN_NONE, c="transposed", tag="ct")
    add(2000, 4100, 64, GEMM128, 1, FIN_NONE, c="interleaved", tag="ci")
    # K split, flat finalize with 2 / 3 / 4 / 8 partials (rr: M must be a multiple of 4)
    add(129, 4100, 512, GEMM128_SPLIT, 2, FIN_FLAT, rr_M=260)
    add(129, 2948, 1000, GEMM128_SPLIT, 3, FIN_FLAT, rr_M=260)
    add(129, 2000, 1024, GEMM128_SPLIT, 4, FIN_FLAT, rr_M=260)
    add(129, 1000, 2050, GEMM128_SPLIT, 8, FIN_FLAT, rr_M=260)
    add(2000, 129, 1024, GEMM128_SPLIT, 4, FIN_FLAT, layouts=[("k", "k")])       # N % 4 != 0
    add(256, 256, 16384, GEMM128_SPLIT, 64, FIN_DEEP)
    add(516, 129, 16384, GEMM128_SPLIT, 52, FIN_DEEP, layouts=[("k", "k")])      # N odd
    # epilogues behind a gemm128 split (the finalize kernels own them)
    add(129, 2000, 1024, GEMM128_SPLIT, 4, FIN_FLAT, layouts=[("k", "r")], bias_i=True, c="transposed", act=ACT_LEAKY, tag="biasi-ct-leaky")
    add(256, 256, 16384, GEMM128_SPLIT, 64, FIN_DEEP, layouts=[("k", "k")], bias_i=True, c="interleaved", act=ACT_TANH, tag="biasi-ci-tanh")
    # a workspace that is short or null: s is cut down; below 128 workgroups the product goes back to the skeleton
    P = 1000 * 2000 * 4
    add(1000, 2000, 1024, GEMM128_SPLIT, 4, FIN_FLAT, layouts=[("k", "k")])
    add(1000, 2000, 1024, GEMM128_SPLIT, 3, FIN_FLAT, layouts=[("k", "k")], ws=4 * P - 1, tag="ws4short")
    add(1000, 2000, 1024, GEMM128_SPLIT, 3, FIN_FLAT, layouts=[("k", "r")], ws=3 * P, tag="ws3")
    add(1000, 2000, 1024, GEMM128_SPLIT, 2, FIN_FLAT, layouts=[("r", "r")], ws=2 * P, tag="ws2")
    add(1000, 2000, 1024, GEMM128, 1, FIN_NONE, layouts=[("k", "k")], ws=P, tag="ws1")
    add(1000, 2000, 1024, GEMM128, 1, FIN_NONE, layouts=[("k", "r")], ws=None, tag="wsnull")
    Q = 129 * 2000 * 4
    for ws, S, tag in ((3 * Q, 3, "ws3"), (2 * Q, 2, "ws2"), (Q, 1, "ws1"), (None, 1, "wsnull")):
        out.append(Gemm("k", "k", 129, 2000, 1024, (SKELETON, 1, 1, S, FIN_FLAT if S > 1 else FIN_NONE), aligned=True, ws=ws, tag=tag))
    return out


def _persistent_cases():
    out = []

    def add(K, layouts=LAYOUTS3, **kw):
        for la, lb in layouts:
            out.append(Gemm(la, lb, 2000, 4100, K, (PERSISTENT, 0, 0, 1, FIN_NONE), **kw))

    for K in (64, 100, 101, 125, 128, 192, 253):          # 528 tiles, ragged last row tile; 2, 4, 4, 4, 4, 6 and 8 stages
        add(K)
    epi = [dict(bias_j=False, tag="nobias"), dict(shift=2, tag="shift2"), dict(act=ACT_LEAKY, tag="leaky"), dict(act=ACT_RELU, tag="relu"),
           dict(act=ACT_TANH, tag="tanh"), dict(act=ACT_SIGMOID, tag="sigmoid")]
    for n, kw in enumerate(epi):
        add(100, layouts=[LAYOUTS3[n % 3]], **kw)
    return out


GEMM_CASES = _skeleton_cases() + _gemm128_cases() + _persistent_cases()
GEMM_BY_ID = {c.id: c for c in GEMM_CASES}
assert len(GEMM_BY_ID) == len(GEMM_CASES)
TWIN_LIMIT = 4e7                                          # M N K the twin's plain loops finish in well under a second
GEMM_TWIN_IDS = [c.id for c in GEMM_CASES if c.M * c.N * c.K <= TWIN_LIMIT] + [      # ... and one aligned case of each larger kind
    "gemm128-kk-1000x2000x65", "gemm128-rr-1000x2000x97", "gemm128-split-kr-129x2000x1024", "gemm128-kr-2000x4100x64-ct",
    "gemm128-kk-2000x4100x64-ci", "persistent-kr-2000x4100x64"]
# one case per kernel kind: the NaN / Inf placement test, and the poison tiers
NONFINITE_IDS = ["skeleton-rk-70x130x40-tanh", "gemm128-kk-1000x2000x65", "gemm128-split-kr-129x2000x1024", "persistent-kr-2000x4100x100"]
POISON_IDS = ["skeleton-kr-1x4100x2050", "gemm128-rr-1000x2000x97", "gemm128-split-kk-129x2948x1000", "persistent-kk-2000x4100x101"]
POISON_TWIN_IDS = ["skeleton-kr-1x4100x2050", "skeleton-kk-1x64x4096-ws5", "gemm128-kk-1000x2000x65", "gemm128-split-kr-129x2000x1024",
                   "persistent-kr-2000x4100x64"]


# ---- operands and references of one sg_gemm variant ---------------------------------------------------------------------------------
def _operands(case, variant):
    M, N, K = case.M, case.N, case.K
    nbj = ((N - 1) >> case.shift) + 1
    if variant == "exact":
        a = torch.randint(-4, 5, (M, K)).float()
        b = torch.randint(-4, 5, (K, N)).float()
        bi, bj = torch.randint(-4, 5, (M,)).float(), torch.randint(-4, 5, (nbj,)).float()
    else:
        a, b = torch.randn(M, K), torch.randn(K, N)
        bi, bj = torch.randn(M), torch.randn(nbj)
        if variant == "scaled":                           # rows of A span 2^-20 .. 2^20
            a = a * torch.exp2(torch.linspace(-20, 20, M).round())[:, None]
    return a, b, (bi if case.bias_i else None), (bj if case.bias_j else None)


def _activate(t, act, slope):
    import torch.nn.functional as F
    return {ACT_NONE: lambda v: v, ACT_LEAKY: lambda v: F.leaky_relu(v, slope), ACT_RELU: torch.relu, ACT_TANH: torch.tanh,
            ACT_SIGMOID: torch.sigmoid}[act](t)


def _reference(case, a, b, bi, bj):
    """float64: the pre-activation sum, the activated result and the bound's magnitude term |A| |B| + |bias_i| + |bias_j|"""
    pre = a.double() @ b.double()
    mag = a.double().abs() @ b.double().abs()
    if bi is not None:
        pre = pre + bi.double()[:, None]
        mag = mag + bi.double().abs()[:, None]
    if bj is not None:
        col = bj.double()[torch.arange(case.N) >> case.shift]
        pre = pre + col[None, :]
        mag = mag + col.abs()[None, :]
    return pre, _activate(pre, case.act, case.slope), mag


def call_gemm(case, a, b, bi, bj, ws):
    """Embeds the operands, makes the call, returns (got [M, N] on the CPU, the plan of the call's own pointers)."""
    from shapegan_amd.lib import ptr, check, stream
    M, N, K = case.M, case.N, case.K
    lda, ldb, sai, sak, sbk, sbj, sci, scj = case.strides()
    oa, ob, oc = case.offsets()
    abuf = embed(a if case.la == "k" else a.t(), lda, oa)
    bbuf = embed(b.t() if case.lb == "k" else b, ldb, ob)
    span = (M - 1) * sci + (N - 1) * scj + 1
    cbuf = torch.full((oc + span + 41,), SENTINEL, dtype=torch.float32, device=OPS.DEV)
    bibuf = None if bi is None else embed_vec(bi)
    bjbuf = None if bj is None else embed_vec(bj)
    ws.poison()
    plan = query_plan(abuf.data_ptr() + 4 * oa, sai, sak, bbuf.data_ptr() + 4 * ob, sbk, sbj, sci, scj, bi is not None, M, N, K,
                      ws.address(), ws.nbytes or 0)
    check(_lib().sg_gemm(ptr(abuf) + 4 * oa, sai, sak, ptr(bbuf) + 4 * ob, sbk, sbj, ptr(cbuf) + 4 * oc, sci, scj,
                         None if bibuf is None else ptr(bibuf) + 12, None if bjbuf is None else ptr(bjbuf) + 12, case.shift, M, N, K,
                         case.act, case.slope, ws.ptr(), ws.nbytes or 0, stream()), "gemm " + case.id)
    got = take_window(cbuf, oc, M, N, sci, scj, case.id)
    ws.check(case.id)
    return got, plan


def check_rounded(got, ref, bound, what, variant):
    got, ref = got.double(), ref.double()
    assert not bool(torch.isnan(got).any()), "%s | %s: NaN in the output" % (what, variant)
    ratio = float(((got - ref).abs() / bound).max())
    print("[gemm-forms] %s | %s | %.3g" % (what, variant, ratio))
    assert ratio <= 1.0, "%s | %s: |got - ref| is %.3g of the bound" % (what, variant, ratio)


def check_exact(got, ref, what):
    assert not bool(torch.isnan(got).any()), what + " | exact: NaN in the output"
    same = got.double() == ref
    print("[gemm-forms] %s | exact | %d of %d elements differ" % (what, int((~same).sum()), same.numel()))
    assert bool(same.all()), "%s | exact: %d element(s) differ from the float64 product, first at %s" % (
        what, int((~same).sum()), (~same).nonzero()[0].tolist())


def body_gemm(case_id):
    case = GEMM_BY_ID[case_id]
    _seed(case.id)
    ws = Workspace(case.ws_bytes())
    variants = (["exact"] if case.act in (ACT_NONE, ACT_LEAKY, ACT_RELU) else []) + ["randn", "scaled"]
    for variant in variants:
        a, b, bi, bj = _operands(case, variant)
        got, plan = call_gemm(case, a, b, bi, bj, ws)
        assert plan["key"] == case.plan, "%s reaches %s, not %s" % (case.id, plan["key"], case.plan)
        _, ref, mag = _reference(case, a, b, bi, bj)
        if variant == "exact":
            check_exact(got, ref, case.id)
        else:
            bound = 1.01 * (case.K + plan["nsplit"] + 4) * EPS * mag + (1e-6 if case.act in (ACT_TANH, ACT_SIGMOID) else 0.0)
            check_rounded(got, ref, bound, case.id, variant)


def check_nonfinite(got, ref, bound, what):
    """Non-finite values exactly where the float64 reference has them (NaN as NaN, +-Inf with its sign), the rest within the bound."""
    got, ref = got.double(), ref.double()
    for name, f in (("NaN", torch.isnan), ("+Inf", torch.isposinf), ("-Inf", torch.isneginf)):
        diff = f(got) != f(ref)
        assert not bool(diff.any()), "%s: %s in %d element(s) where the reference has none, or the reverse; first at %s" % (
            what, name, int(diff.sum()), diff.nonzero()[0].tolist())
    fin = torch.isfinite(ref)
    assert int(fin.sum()) > 0 and int((~fin).sum()) > 0
    ratio = float(((got - ref).abs()[fin] / bound[fin]).max())
    print("[gemm-forms] %s | nonfinite | %.3g" % (what, ratio))
    assert ratio <= 1.0, what


def body_gemm_nonfinite(case_id):
    """One NaN in A and one Inf in B: row i0 of C is NaN, column j1 is +-Inf by the sign of A[:, k1], everything else is finite."""
    base = GEMM_BY_ID[case_id]
    case = Gemm(base.la, base.lb, base.M, base.N, base.K, base.plan, aligned=base.aligned, ws=base.ws, bias_i=False, bias_j=False)
    _seed(case.id + "nonfinite")
    a, b, _, _ = _operands(case, "randn")
    i0, k0, k1, j1 = case.M - 2, case.K - 1, case.K // 2, case.N - 3
    a[i0, k0] = float("nan")
    b[k1, j1] = float("inf")
    ws = Workspace(case.ws_bytes())
    got, plan = call_gemm(case, a, b, None, None, ws)
    assert plan["key"] == case.plan, (plan["key"], case.plan)
    ref = a.double() @ b.double()
    mag = torch.nan_to_num(a.double().abs(), nan=0.0) @ torch.nan_to_num(b.double().abs(), posinf=0.0)
    check_nonfinite(got, ref, 1.01 * (case.K + plan["nsplit"] + 4) * EPS * mag, case.id)


# ---- sg_gemm_nt / sg_gemm_nt_batched / sg_gemm_nt_batched_lnrelu --------------------------------------------------------------------
class GemmNt(object):
    """entry: 'nt' (sg_gemm_nt), 'batched', 'lnrelu'.  plan = (direct, nsplit) claimed."""

    def __init__(self, entry, batch, M, N, K, plan):
        self.entry, self.batch, self.M, self.N, self.K, self.plan = entry, batch, M, N, K, tuple(plan)
        self.id = "%s-b%d-%dx%dx%d" % (entry, batch, M, N, K)


NT_CASES = (
    [GemmNt("nt", 1, 129, 70, K, (True, 1)) for K in (1, 31, 64, 65, 67, 68, 95, 96, 97, 100, 129, 511)] +      # direct: K < 512
    [GemmNt("nt", 1, M, N, 515, (False, 2)) for M, N in ((1, 1), (70, 128), (128, 70), (1, 260), (260, 1))] +
    [GemmNt("nt", 1, M, N, 800, (False, 3)) for M, N in ((129, 256), (256, 129), (260, 260))] +
    [GemmNt("nt", 1, 3, 5, 65536, (False, 256)), GemmNt("nt", 1, 70, 129, 16400, (False, 57)),
     GemmNt("batched", 1, 70, 129, 100, (True, 1)), GemmNt("batched", 2, 70, 129, 100, (False, 1)),
     GemmNt("batched", 8, 129, 70, 101, (False, 1)), GemmNt("batched", 2, 128, 128, 1000, (False, 3)),
     GemmNt("batched", 8, 70, 260, 1003, (False, 3)), GemmNt("batched", 1, 256, 256, 515, (False, 2)),
     GemmNt("lnrelu", 1, 70, 129, 100, (True, 1)), GemmNt("lnrelu", 2, 129, 260, 1003, (False, 3)),
     GemmNt("lnrelu", 8, 1, 70, 515, (False, 2))])
NT_BY_ID = {c.id: c for c in NT_CASES}
assert len(NT_BY_ID) == len(NT_CASES)
NT_NONFINITE_ID = "nt-b1-260x260x800"
NT_POISON_IDS = ["nt-b1-70x128x515", "lnrelu-b2-129x260x1003"]


def _arr(values):
    return (ctypes.c_long * len(values))(*values)


def call_gemm_nt(case, As, Bs, gammas, betas, ws_short=0):
    """As[b] [M, K], Bs[b] [N, K] (gammas / betas [b][N] for lnrelu).  Returns ([got_b], plan, return code)."""
    from shapegan_amd.lib import ptr, stream
    batch, M, N, K = case.batch, case.M, case.N, case.K
    lda, ldb = _ld(K, False), _ld(K + 2, False)
    assert lda != ldb and lda % 4 and ldb % 4
    plan = query_nt_plan(batch, M, N, K)
    # the members' operands behind one another in one NaN buffer each, with gaps
    a_off = [3 + b * ((M + 4) * lda + 7) for b in range(batch)]       # (four NaN rows behind every member)
    b_off = [5 + b * ((N + 4) * ldb + 9) for b in range(batch)]
    abuf = torch.full((a_off[-1] + (M + 4) * lda + 11,), float("nan"))
    bbuf = torch.full((b_off[-1] + (N + 4) * ldb + 11,), float("nan"))
    for m in range(batch):
        abuf[a_off[m]:a_off[m] + M * lda].view(M, lda)[:, :K] = As[m]
        bbuf[b_off[m]:b_off[m] + N * ldb].view(N, ldb)[:, :K] = Bs[m]
    abuf, bbuf = abuf.to(OPS.DEV), bbuf.to(OPS.DEV)
    ldc = [N + 1 + 2 * m for m in range(batch)]          # a different row stride per member
    c_off, at = [], 3
    for m in range(batch):
        c_off.append(at)
        at += M * ldc[m] + 6
    cbuf = torch.full((at + 13,), SENTINEL, dtype=torch.float32, device=OPS.DEV)
    nbytes = plan["ws_bytes"] - ws_short
    ws = Workspace(nbytes if plan["ws_bytes"] else None)
    lib = _lib()
    if case.entry == "nt":
        rc = lib.sg_gemm_nt(ptr(abuf) + 4 * a_off[0], lda, ptr(bbuf) + 4 * b_off[0], ldb, ptr(cbuf) + 4 * c_off[0], ldc[0], M, N, K,
                            ws.ptr(), ws.nbytes or 0, stream())
    elif case.entry == "batched":
        rc = lib.sg_gemm_nt_batched(ptr(abuf), _arr(a_off), lda, ptr(bbuf), _arr(b_off), ldb, ptr(cbuf), _arr(c_off), _arr(ldc), batch, M, N,
                                    K, ws.ptr(), ws.nbytes or 0, stream())
    else:
        g_off = [3 + m * (N + 4) for m in range(batch)]
        gbuf = torch.full((g_off[-1] + N + 5,), float("nan"))
        tbuf = gbuf.clone()
        for m in range(batch):
            gbuf[g_off[m]:g_off[m] + N] = gammas[m]
            tbuf[g_off[m]:g_off[m] + N] = betas[m]
        gbuf, tbuf = gbuf.to(OPS.DEV), tbuf.to(OPS.DEV)
        rc = lib.sg_gemm_nt_batched_lnrelu(ptr(abuf), _arr(a_off), lda, ptr(bbuf), _arr(b_off), ldb, ptr(gbuf), ptr(tbuf), _arr(g_off),
                                           ptr(cbuf), _arr(c_off), _arr(ldc), batch, M, N, K, ws.ptr(), ws.nbytes or 0, stream())
    if OPS.DEV != "cpu":
        torch.cuda.synchronize()
    ws.check(case.id)
    if rc != 0:
        assert bool((cbuf == SENTINEL).all()), case.id + ": a refused call wrote to C"
        return None, plan, rc
    gots = []
    for m in range(batch):                                # (take_window re-fills each window: the last call sees all of them gone)
        view = cbuf.as_strided((M, N), (ldc[m], 1), c_off[m])
        gots.append(view.clone().cpu())
        view.fill_(SENTINEL)
    assert bool((cbuf == SENTINEL).all()), case.id + ": an element outside the output windows was written"
    return gots, plan, rc


def _nt_operands(case, variant):
    batch, M, N, K = case.batch, case.M, case.N, case.K
    if variant == "exact":
        r = lambda *s: torch.randint(-4, 5, s).float()  # noqa: E731
        return ([r(M, K) for _ in range(batch)], [r(N, K) for _ in range(batch)],
                [torch.randint(1, 3, (N,)).float() for _ in range(batch)], [torch.randint(-2, 3, (N,)).float() for _ in range(batch)])
    As, Bs = [torch.randn(M, K) for _ in range(batch)], [torch.randn(N, K) for _ in range(batch)]
    if variant == "scaled":
        As = [a * torch.exp2(torch.linspace(-20, 20, M).round())[:, None] for a in As]
    return As, Bs, [torch.rand(N) + 0.5 for _ in range(batch)], [torch.randn(N) * 0.3 for _ in range(batch)]


def _nt_reference(case, a, b, g, t):
    """float64 product and magnitude term.  lnrelu: B' = relu(gamma x + beta) is formed in fp32 by the kernel, once rounded when fused,
    twice when not: its error is bounded relative to |gamma| |x| + |beta|, which therefore is the magnitude of B here (one of the
    bound's four spare terms)."""
    bd = b.double()
    if case.entry == "lnrelu":
        mag_b = g.double().abs()[:, None] * bd.abs() + t.double().abs()[:, None]
        bd = torch.relu(g.double()[:, None] * bd + t.double()[:, None])
    else:
        mag_b = bd.abs()
    return a.double() @ bd.t(), a.double().abs() @ mag_b.t()


def body_gemm_nt(case_id):
    case = NT_BY_ID[case_id]
    _seed(case.id)
    for variant in ("exact", "randn", "scaled"):
        As, Bs, gs, ts = _nt_operands(case, variant)
        gots, plan, rc = call_gemm_nt(case, As, Bs, gs, ts)
        assert rc == 0, case.id
        assert (plan["direct"], plan["nsplit"]) == case.plan, "%s plans %s" % (case.id, plan)
        for m in range(case.batch):
            ref, mag = _nt_reference(case, As[m], Bs[m], gs[m], ts[m])
            what = "%s[%d]" % (case.id, m)
            if variant == "exact":
                check_exact(gots[m], ref, what)
            else:
                check_rounded(gots[m], ref, 1.01 * (case.K + plan["nsplit"] + 4) * EPS * mag, what, variant)


def body_gemm_nt_nonfinite():
    case = NT_BY_ID[NT_NONFINITE_ID]
    _seed(case.id + "nonfinite")
    As, Bs, gs, ts = _nt_operands(case, "randn")
    As[0][case.M - 2, case.K - 1] = float("nan")
    Bs[0][case.N - 3, case.K // 2] = float("inf")
    gots, plan, rc = call_gemm_nt(case, As, Bs, gs, ts)
    assert rc == 0
    ref = As[0].double() @ Bs[0].double().t()
    mag = torch.nan_to_num(As[0].double().abs(), nan=0.0) @ torch.nan_to_num(Bs[0].double().abs(), posinf=0.0).t()
    check_nonfinite(gots[0], ref, 1.01 * (case.K + plan["nsplit"] + 4) * EPS * mag, case.id)


def body_gemm_nt_short_workspace(case_id):
    """A workspace one byte short: SG_ERR_WORKSPACE, and C untouched (call_gemm_nt asserts the latter).  The twin takes no workspace."""
    case = NT_BY_ID[case_id]
    _seed(case.id)
    As, Bs, gs, ts = _nt_operands(case, "randn")
    gots, plan, rc = call_gemm_nt(case, As, Bs, gs, ts, ws_short=1)
    assert not plan["direct"] and rc == SG_ERR_WORKSPACE and gots is None, (plan, rc)
    from shapegan_amd import lib as L
    assert b"workspace too small" in L._load_hip().sg_last_error()


# ---- reductions ---------------------------------------------------------------------------------------------------------------------
def _values(shape, variant, scaled_dim=0):
    if variant == "exact":
        return torch.randint(-4, 5, shape).float()
    x = torch.randn(*shape)
    if variant == "scaled":
        e = torch.exp2(torch.linspace(-20, 20, shape[scaled_dim]).round())
        x = x * (e[:, None] if scaled_dim == 0 else e[None, :])
    return x


def _check_sums(got, ref, mag, length, what, variant):
    """1.01 (len + 8) 2^-24 sum |x|: a len-term fp32 sum in any order (tree or serial) with room for the cross-lane steps; `length` is
    a number or a tensor that broadcasts against the outputs (sg_segsum: each segment's own length)"""
    if variant == "exact":
        check_exact(got, ref, what)
    else:
        bound = 1.01 * (length + 8) * EPS * mag
        bound = torch.where(bound > 0, bound, torch.full_like(bound, 1e-300))
        check_rounded(got, ref, bound, what, variant)


# (both sides of the wave / workgroup switch; 4092 and 4100: the float4 stream's tail loop with 64 and with 256 lanes)
ROWSUM_CASES = [(1023, 4096), (1024, 4096), (1024, 4097), (1025, 1), (3, 70001), (1024, 63), (5, 4096), (1024, 4092), (5, 4100)]


def body_rowsum(rows, length):
    from shapegan_amd.lib import ptr, check, stream
    what = "rowsum-%dx%d" % (rows, length)
    _seed(what)
    for variant in ("exact", "randn", "scaled"):
        for ld, off in ((length + 3, 5), ((length + 3) // 4 * 4 + 4, 8)):       # the scalar stream and the float4 stream (len % 4 == 0)
            x = _values((rows, length), variant)
            xbuf = embed(x, ld, off)
            out = torch.full((rows + 9,), SENTINEL, dtype=torch.float32, device=OPS.DEV)
            check(_lib().sg_rowsum(ptr(xbuf) + 4 * off, ptr(out) + 16, rows, length, ld, stream()), what)
            got = take_window(out, 4, rows, 1, 1, 1, what)[:, 0]
            _check_sums(got, x.double().sum(1), x.double().abs().sum(1), length, "%s-ld%d" % (what, ld), variant)


ROWSUM_MULTI_CASES = [(ndst, rpd, length, strided) for ndst, rpd, length, strided in
                      [(1, 1, 1, False), (7, 37, 63, True), (8, 37, 64, False), (8, 1, 65, True), (7, 1, 257, False), (1, 37, 5000, True),
                       (8, 37, 5000, True)]]


def body_rowsum_multi(ndst, rpd, length, strided):
    from shapegan_amd.lib import ptr, check, stream, note_device
    what = "rowsum_multi-%d-%d-%d-%s" % (ndst, rpd, length, "strided" if strided else "unit")
    _seed(what)
    strides = [1 + 2 * (d % 3) for d in range(ndst)] if strided else [1] * ndst        # 1, 3, 5, 1, ...
    for variant in ("exact", "randn", "scaled"):
        ld, off = (length + 3) // 4 * 4 + 4, 8
        x = _values((ndst * rpd, length), variant)
        xbuf = embed(x, ld, off)
        starts, at = [], 2
        for d in range(ndst):
            starts.append(at)
            at += (rpd - 1) * strides[d] + 1 + 3
        out = torch.full((at + 5,), SENTINEL, dtype=torch.float32, device=OPS.DEV)
        note_device(out)
        outs = (ctypes.c_void_p * ndst)(*[out.data_ptr() + 4 * s for s in starts])
        check(_lib().sg_rowsum_multi(ptr(xbuf) + 4 * off, outs, _arr(strides) if strided else None, ndst, rpd, length, ld, stream()), what)
        got = []
        for d in range(ndst):
            view = out.as_strided((rpd,), (strides[d],), starts[d])
            got.append(view.clone().cpu())
            view.fill_(SENTINEL)
        assert bool((out == SENTINEL).all()), what + ": an element outside the destinations was written"
        _check_sums(torch.cat(got), x.double().sum(1), x.double().abs().sum(1), length, what, variant)


SEGSUM_CASES = [(1, 1, (1000,)), (3, 5, (0, 1, 63, 64, 65)), (7, 5, (1000, 0, 65, 1, 64)), (2, 1, (0,)), (1025, 5, (63, 0, 0, 64, 1))]


def body_segsum(rows, nseg, lengths):
    from shapegan_amd.lib import ptr, check, stream
    what = "segsum-%d-%s" % (rows, "_".join(str(v) for v in lengths))
    _seed(what)
    assert len(lengths) == nseg
    seg_off = [0]
    for v in lengths:
        seg_off.append(seg_off[-1] + v)
    total = max(seg_off[-1], 1)
    for variant in ("exact", "randn", "scaled"):
        ld, off = total + 6, 5
        x = _values((rows, total), variant)
        xbuf = embed(x, ld, off)
        offs = torch.tensor(seg_off, dtype=torch.int64, device=OPS.DEV)
        out = torch.full((rows * nseg + 9,), SENTINEL, dtype=torch.float32, device=OPS.DEV)
        check(_lib().sg_segsum(ptr(xbuf) + 4 * off, ptr(out) + 16, rows, ld, ptr(offs), nseg, stream()), what)
        got = take_window(out, 4, rows, nseg, nseg, 1, what)
        xd = x.double()
        ref = torch.stack([xd[:, seg_off[s]:seg_off[s + 1]].sum(1) for s in range(nseg)], 1)
        mag = torch.stack([xd[:, seg_off[s]:seg_off[s + 1]].abs().sum(1) for s in range(nseg)], 1)
        _check_sums(got, ref, mag, torch.tensor(lengths, dtype=torch.float64)[None, :], what, variant)       # each segment's own length


COLSUM_CASES = [(1, 1), (255, 63), (256, 64), (257, 65), (1, 130), (257, 130), (9, 64), (8, 65)]


def body_colsum(rows, cols):
    from shapegan_amd.lib import ptr, check, stream
    what = "colsum-%dx%d" % (rows, cols)
    _seed(what)
    for variant in ("exact", "randn", "scaled"):
        ld, off = cols + 3, 5
        x = _values((rows, cols), variant, scaled_dim=1)
        xbuf = embed(x, ld, off)
        out = torch.full((cols + 9,), SENTINEL, dtype=torch.float32, device=OPS.DEV)
        check(_lib().sg_colsum(ptr(xbuf) + 4 * off, ptr(out) + 16, rows, cols, ld, stream()), what)
        got = take_window(out, 4, 1, cols, cols, 1, what)[0]
        _check_sums(got, x.double().sum(0), x.double().abs().sum(0), rows, what, variant)
