"""GPU: the perturbed form of rsa_spmm_csr (ops.spmm_csr(noise=...), SimGCL's layer) -- its uniforms against torch.rand_like from
the same generator state, every output against the float64 referee of tests/simgcl_referee.py, and the properties the header
promises: rows without edges stay 0, two runs are bit-equal, a row's perturbation does not depend on the plan, and noise_eps = 0
is the plain product."""
import ctypes

import pytest
import torch

import simgcl_referee as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS, CAP = 0.1, 1e-4


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


def on_dev(case):
    return {k: None if v is None else v.to(DEV) for k, v in case.items()}


def reserve(ra, numel, seed):
    """A PhiloxCall for one rand_like over ``numel`` outputs from the seeded default generator."""
    torch.manual_seed(seed)
    return ra.rng.reserve(numel, 4, torch.device(DEV))


@pytest.mark.parametrize('rows,d', [(70, 4), (70, 36), (70, 64), (70, 128), (70, 256), (8200, 256)])
def test_uniforms_are_torch_rand_like(ra, rows, d):
    """One edge per row (row r reads column r % 7); 8200 x 256 is more than 4 x 524288 elements: past the first Philox round
    of the largest grid torch launches on this device."""
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    indptr = torch.arange(rows + 1, device=DEV)
    indices = (torch.arange(rows, device=DEV) % 7).int()
    x = torch.randn(7, d, device=DEV)
    if rows > 70:
        cu, mt = ra.rng.device_props(DEV)
        assert rows * d > 4 * ra.rng.grid_threads(rows * d, cu, mt)
    plan = ra.ops.spmm_plan(indptr, 8)
    torch.manual_seed(77)
    want = torch.rand_like(torch.empty(rows, d, device=DEV))
    want_offset = gen.get_offset()
    torch.manual_seed(77)
    u = torch.full((rows, d), -1.0, device=DEV)
    y = ra.ops.spmm_csr(indptr, indices, None, x, plan=plan, noise=ra.rng.reserve(rows * d, 4, torch.device(DEV)), noise_eps=EPS, noise_out=u)
    assert torch.equal(u, want) and gen.get_offset() == want_offset
    # and the output is the row moved by eps along sign(row) * u / ||u|| (x has no zero)
    s = x[indices.long()]
    moved = (y - s).double()
    ref = torch.sign(s).double() * torch.nn.functional.normalize(u.double(), dim=-1) * EPS
    assert float((moved - ref).abs().max()) < 1e-6


VARIANTS = ['y', 'y scaled', 'acc', 'acc scaled', 'y and acc', 'acc_out']


@pytest.mark.parametrize('d', [4, 36, 64, 128, 256])
@pytest.mark.parametrize('variant', VARIANTS)
def test_outputs_stay_inside_the_bound(ra, d, variant):
    """Chunk 8 over rows of 0, 1, 7, 8, 9, 16, 17, ... edges and one row of half the edges (split into many pieces)."""
    c = on_dev(sc.ragged_case(d))
    R = c['indptr'].numel() - 1
    plan = ra.ops.spmm_plan(c['indptr'], 8)
    assert plan.n_split >= 4
    row_scale = c['row_scale'] if 'scaled' in variant else None
    want_y, want_acc = 'y' in variant, 'acc' in variant
    k = 0.25 if want_acc else 1.0
    y = torch.full((R, d), 7.0, device=DEV) if want_y else None
    acc = c['acc'].clone() if want_acc else None
    acc_out = torch.full((R, d), 7.0, device=DEV) if variant == 'acc_out' else None
    u = torch.empty(R, d, device=DEV)

    def run():
        return ra.ops.spmm_csr(c['indptr'], c['indices'], c['values'], c['x'], plan=plan, row_scale=row_scale, y=y, acc=acc, acc_scale=k,
                               acc_out=acc_out, noise=reserve(ra, R * d, 5), noise_eps=EPS, noise_out=u)

    run()
    got_acc = None if not want_acc else (acc_out if acc_out is not None else acc)
    if variant == 'acc_out':
        assert torch.equal(acc, c['acc'])                                           # acc_in is only read
    ref = sc.layer(c['indptr'], c['indices'], c['values'], c['x'], u, EPS, row_scale=row_scale, acc=c['acc'] if want_acc else None, acc_scale=k)
    j = sc.judge(ref, got_y=y, got_acc=got_acc)
    print(f'd = {d}, {variant}: |got - ref| / bound = {j["ratio"]:.3f}, ambiguous share {j["share"]:.2e}')
    assert j['ratio'] <= 1.0 and j['share'] <= CAP
    deg = c['indptr'][1:] - c['indptr'][:-1]
    if want_y:
        empty = y[deg == 0]
        assert empty.numel() and bool((empty.view(torch.int32) == 0).all())          # rows without edges: +0 in every bit
        assert float((y - ref['s'].float()).abs().max()) > 0.01 * EPS                # the noise is there
    # two runs are bit-equal
    first = [t.clone() for t in (y, got_acc, u) if t is not None]
    if want_acc and acc_out is None:
        acc.copy_(c['acc'])
    run()
    assert all(torch.equal(a, b) for a, b in zip(first, [t for t in (y, got_acc, u) if t is not None]))


@pytest.mark.parametrize('d', [4, 36, 64, 256])
def test_the_perturbation_of_a_row_does_not_depend_on_the_plan(ra, d):
    """Small-integer x and unit weights: every partial sum is exact, so the rows' sums are the same bits under any plan, and so
    must be their perturbed values -- the uniforms, q and the one application per row cannot depend on how a row is cut."""
    c = on_dev(sc.ragged_case(d, integer=True))
    R = c['indptr'].numel() - 1
    longest = int((c['indptr'][1:] - c['indptr'][:-1]).max())
    out = {}
    for chunk in (4, longest + 1):
        plan = ra.ops.spmm_plan(c['indptr'], chunk)
        assert (plan.n_split > 0) == (chunk == 4)
        y, acc, u = torch.empty(R, d, device=DEV), c['acc'].clone(), torch.empty(R, d, device=DEV)
        ra.ops.spmm_csr(c['indptr'], c['indices'], None, c['x'], plan=plan, y=y, acc=acc, acc_scale=0.5, noise=reserve(ra, R * d, 6),
                        noise_eps=EPS, noise_out=u)
        out[chunk] = (y, acc, u)
    assert all(torch.equal(a, b) for a, b in zip(out[4], out[longest + 1]))
    plain = ra.ops.spmm_csr(c['indptr'], c['indices'], None, c['x'], plan=ra.ops.spmm_plan(c['indptr'], 4))
    # once per row: the row moved by eps * u / ||u|| on its non-zero elements, split or not
    moved = (out[4][0] - plain).double().abs()
    want = (plain != 0).double() * torch.nn.functional.normalize(out[4][2].double(), dim=-1) * EPS
    assert float((moved - want).abs().max()) < 1e-4 * EPS + 2.0 ** -23 * float(plain.abs().max())


@pytest.mark.parametrize('d', [36, 64])
def test_noise_eps_zero_is_the_call_without_the_fields(ra, d):
    c = on_dev(sc.ragged_case(d))
    R = c['indptr'].numel() - 1
    plan = ra.ops.spmm_plan(c['indptr'], 8)
    y0, acc0 = torch.empty(R, d, device=DEV), c['acc'].clone()
    ra.ops.spmm_csr(c['indptr'], c['indices'], c['values'], c['x'], plan=plan, row_scale=c['row_scale'], y=y0, acc=acc0, acc_scale=0.5,
                    noise_eps=0.0)
    # the argument block as a caller built against the header of before passes it: cut before the noise fields (which hold junk)
    nat, ptr = ra._native, ra._native.ptr
    y1, acc1 = torch.empty(R, d, device=DEV), c['acc'].clone()
    partials = plan.partials(d, torch.device(DEV, torch.cuda.current_device()))
    a = nat.SpmmArgs()
    a.indptr, a.indices, a.values = ptr(c['indptr']), ptr(c['indices']), ptr(c['values'])
    a.n_rows, a.n_cols, a.nnz, a.dim = R, c['x'].shape[0], c['indices'].numel(), d
    a.x, a.row_scale, a.y, a.acc_in, a.acc_out, a.acc_scale = ptr(c['x']), ptr(c['row_scale']), ptr(y1), ptr(acc1), ptr(acc1), 0.5
    a.chunk, a.n_split, a.n_parts = plan.chunk, plan.n_split, plan.n_parts
    a.plan, a.plan_len, a.partials, a.partials_bytes = ptr(plan.table), plan.table.numel(), ptr(partials), partials.numel() * 4
    a.noise_eps, a.noise_grid_threads, a.noise_seed = 0.5, 256, 99
    a.size = nat.SpmmArgs.noise_eps.offset
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert nat.lib().rsa_spmm_csr(ctypes.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(acc0, acc1)
    with pytest.raises(ValueError, match='without noise_eps'):
        ra.ops.spmm_csr(c['indptr'], c['indices'], c['values'], c['x'], plan=plan, noise=reserve(ra, R * d, 1))
    with pytest.raises(TypeError, match='PhiloxCall'):
        ra.ops.spmm_csr(c['indptr'], c['indices'], c['values'], c['x'], plan=plan, noise_eps=0.1)
