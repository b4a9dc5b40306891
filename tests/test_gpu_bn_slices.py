"""-m gpu: the channel-sliced geometry of the BatchNorm streaming kernels (bn_apply_kernel / bn_bwd_dx_kernel, csrc/norm.hip: a block owns
a slice of cs channels x a run of rows and derives the per-channel constants of its slice only).

 * bit identity: every form of emrt_bn_apply / emrt_bn_apply_join / emrt_bn_bwd_dx gives the same bits with bn_slice_c = 0 (the automatic
   rule), with every slice width forced (64, 128, 256) and with the whole-row geometry (bn_slice_c >= C).  dgamma, dbeta and the running
   statistics start from non-zero values, so a channel whose once-per-layer duty ran twice or never differs.
 * reference: the same channel counts through bn_train_case (per-channel statistics, float64 reference) at its existing bounds, so the
   sliced path itself is right and not only equal to the old one.

Rows: 1, one less and one more than the rows a block takes per pass (4 / 8 / 16 at slices of 256 / 128 / 64 channels), a ragged few hundred that
leave the last row block partial, and 1111 (several passes per block at every width)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                     # noqa: E402
from emrt_amd.functional import P, BN_REPLICAS                # noqa: E402
from emrt_amd.runtime import F32, BF16                        # noqa: E402
from tests.hip_utils import init                              # noqa: E402
from tests.test_gpu_kernels import bn_train_case              # noqa: E402

DTYPES = [F32, BF16]
CHANNELS = [64, 128, 256, 512, 1024, 2048, 1028]      # one slice | 2-32 slices | no slice width divides it: whole rows
ROWS = [1, 3, 5, 7, 9, 15, 17, 333, 1111]
WHOLE = 1 << 20                                       # bn_slice_c >= C: whole rows
WIDTHS = [0, 64, 128, 256]
EPS, MOM = 1e-5, 0.9


def replica_sums(cols):
    """[M][2C] fp64 columns -> the [8][2C] replica layout of the BatchNorm sums (replica k: rows k, k + 8, ...)."""
    out = torch.zeros(BN_REPLICAS, cols.shape[1], dtype=torch.float64)
    for k in range(BN_REPLICAS):
        out[k] = cols[k::BN_REPLICAS].sum(0)
    return out.reshape(-1)


class Inputs:
    def __init__(self, c, C, M, seed):
        g = torch.Generator().manual_seed(seed)
        td = c.tdtype
        scale = torch.rand(C, generator=g) * 1.5 + 0.5
        shift = torch.rand(C, generator=g) * 4 - 2

        def m(t):
            return t.to(td).to(c.device)

        x = (torch.randn(M, C, generator=g) * scale + shift).to(td)
        r = (torch.randn(M, C, generator=g) * scale.flip(0) - shift).to(td)
        dy = torch.randn(M, C, generator=g).to(td)
        y = torch.randn(M, C, generator=g).to(td)            # a ReLU output stand-in: the sign is the mask
        self.x, self.res, self.dy, self.y = m(x), m(r), m(dy), m(y)
        xd, rd, dd = x.double(), r.double(), dy.double()
        self.sums = replica_sums(torch.cat([xd, xd * xd], 1)).to(c.device)
        self.r_sums = replica_sums(torch.cat([rd, rd * rd], 1)).to(c.device)
        self.bsums = replica_sums(torch.cat([dd, dd * xd], 1)).to(c.device)           # (sum dy, sum dy * x): every backward form reads them its own way
        self.lsums = replica_sums(torch.cat([dd * 0.5, dd * rd], 1)).to(c.device)     # "this rank's" sums of the SyncBatchNorm form
        f = dict(device=c.device, dtype=torch.float32)
        self.gamma = (torch.rand(C, generator=g) + 0.5).to(**f)
        self.beta = (torch.randn(C, generator=g) * 0.2).to(**f)
        self.r_gamma = (torch.rand(C, generator=g) + 0.5).to(**f)
        self.r_beta = (torch.randn(C, generator=g) * 0.2).to(**f)
        self.mean = shift.to(**f)
        self.invstd = (1.0 / scale).to(**f)
        self.run_mean0 = (torch.randn(C, generator=g) * 0.3 + 0.1).to(**f)            # non-zero starting values
        self.run_var0 = (torch.rand(C, generator=g) + 0.5).to(**f)
        self.dgamma0 = (torch.randn(C, generator=g) + 3.0).to(**f)
        self.dbeta0 = (torch.randn(C, generator=g) - 3.0).to(**f)


def run_forms(L, c, inp, C, M):
    """every form once under the current knobs -> {name: tensor}"""
    out = {}
    f32 = dict(device=c.device, dtype=torch.float32)

    def fresh(n=C):
        return torch.full((n,), 7.0, **f32)

    def keep(tag, **tensors):
        for k, v in tensors.items():
            if v is not None:
                out["%s.%s" % (tag, k)] = v

    for res in (False, True):
        for relu in (0, 1):
            y, mean, invstd = torch.empty_like(inp.x), fresh(), fresh()
            rm, rv = inp.run_mean0.clone(), inp.run_var0.clone()
            L.call("emrt_bn_apply", P(inp.x), C, P(inp.res) if res else None, C if res else 0, P(y), C, P(inp.sums), float(M), EPS, MOM, P(mean), P(invstd),
                   P(rm), P(rv), P(inp.gamma), P(inp.beta), M, C, relu, c.dtype, c.stream)
            keep("train res%d relu%d" % (res, relu), y=y, mean=mean, invstd=invstd, run_mean=rm, run_var=rv)
    for res, relu in ((False, 0), (True, 1)):
        y = torch.empty_like(inp.x)
        rm, rv = inp.run_mean0.clone(), inp.run_var0.clone()
        L.call("emrt_bn_apply", P(inp.x), C, P(inp.res) if res else None, C if res else 0, P(y), C, None, 1.0, EPS, MOM, None, None,
               P(rm), P(rv), P(inp.gamma), P(inp.beta), M, C, relu, c.dtype, c.stream)
        keep("eval res%d relu%d" % (res, relu), y=y, run_mean=rm, run_var=rv)
    y, mean, invstd, r_mean, r_invstd = torch.empty_like(inp.x), fresh(), fresh(), fresh(), fresh()
    rm, rv, r_rm, r_rv = inp.run_mean0.clone(), inp.run_var0.clone(), inp.run_var0.clone(), inp.run_mean0.abs() + 0.25
    L.call("emrt_bn_apply_join", P(inp.x), C, P(inp.res), C, P(y), C, P(inp.sums), float(M), EPS, MOM, P(mean), P(invstd), P(rm), P(rv), P(inp.gamma),
           P(inp.beta), P(inp.r_sums), float(M), EPS, MOM, P(r_mean), P(r_invstd), P(r_rm), P(r_rv), P(inp.r_gamma), P(inp.r_beta), M, C, 1, c.dtype, c.stream)
    keep("join", y=y, mean=mean, invstd=invstd, run_mean=rm, run_var=rv, r_mean=r_mean, r_invstd=r_invstd, r_run_mean=r_rm, r_run_var=r_rv)
    # (name, y mask, dres, local sums, beta_y_moments, sums_vs_x, mask_beta)
    forms = [("bwd y", True, True, False, False, 0, False), ("bwd beta_y_moments", True, False, False, True, 0, False),
             ("bwd sums_vs_x", True, True, False, False, 1, False), ("bwd mask_beta", False, False, False, False, 0, True),
             ("bwd local_sums", True, True, True, False, 0, False), ("bwd no mask", False, False, False, False, 0, False)]
    for name, ymask, want_dres, local, beta_y, vs_x, mask_beta in forms:
        dx = torch.empty_like(inp.x)
        dres = torch.empty_like(inp.x) if want_dres else None
        dgamma, dbeta = inp.dgamma0.clone(), inp.dbeta0.clone()
        L.call("emrt_bn_bwd_dx", P(inp.x), C, P(inp.dy), C, P(inp.y) if ymask else None, C if ymask else 0, P(dx), C, P(dres), C, P(inp.mean), P(inp.invstd),
               P(inp.gamma), P(inp.bsums), P(inp.lsums) if local else None, float(M), P(dgamma), P(dbeta), M, C, P(inp.beta) if beta_y else None, vs_x,
               P(inp.beta) if mask_beta else None, c.dtype, c.stream)
        keep(name, dx=dx, dres=dres, dgamma=dgamma, dbeta=dbeta)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", CHANNELS)
def test_sliced_geometry_is_bit_identical_to_whole_rows(dtype, C):
    c = init(dtype)
    L = _lib.lib()
    old = L.set_tuning("bn_slice_c", 0)
    try:
        for M in ROWS:
            inp = Inputs(c, C, M, seed=1000 + M)
            L.set_tuning("bn_slice_c", WHOLE)
            want = run_forms(L, c, inp, C, M)
            for k, v in want.items():
                assert torch.isfinite(v.float()).all(), "C %d M %d %s: non-finite values in the whole-row result" % (C, M, k)
            for width in WIDTHS:
                L.set_tuning("bn_slice_c", width)
                got = run_forms(L, c, inp, C, M)
                assert got.keys() == want.keys()
                for k in want:
                    assert torch.equal(got[k], want[k]), "C %d M %d bn_slice_c %d: %s differs from the whole-row geometry in %d elements" % (
                        C, M, width, k, int((got[k] != want[k]).sum()))
            # the duties ran: the accumulators moved off their starting values in every channel, the saved statistics were written
            assert not torch.equal(want["bwd y.dgamma"], inp.dgamma0) and (want["train res0 relu0.mean"] != 7.0).all()
    finally:
        L.set_tuning("bn_slice_c", old)


# The reference helper draws its own input and needs a batch statistic torch can form and a standard deviation above 0.1 in every one of up
# to 2048 channels (population_floor): rows from 15 up (1 x 3 x 5, 1 x 1 x 17: one less / one more than the 16 rows per pass of the 64-channel
# slices; 3 x 3 x 37 and 1 x 11 x 101: ragged, several row blocks).  The rows below that are covered by the bit-identity test above only.
REF_SHAPES = [(1, 3, 5), (1, 1, 17), (3, 3, 37), (1, 11, 101)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", CHANNELS)
def test_sliced_geometry_against_float64(dtype, C):
    L = _lib.lib()
    old = L.set_tuning("bn_slice_c", 0)             # the automatic rule is what runs
    try:
        for i, (N, H, W) in enumerate(REF_SHAPES):
            relu, with_res = ((True, True), (False, False), (True, False))[i % 3]
            bn_train_case(dtype, N, H, W, C, relu, with_res, per_channel=True, ref=torch.float64)
    finally:
        L.set_tuning("bn_slice_c", old)
