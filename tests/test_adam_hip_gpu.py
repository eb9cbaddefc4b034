"""`fcvsr_adam_multi` / `HipAdam`: the one-launch Adam equals its numpy float32 specification (`adam_step_host`) bit for bit, for every
alignment of a tensor in the flat buffers, writes nothing outside its tensors, advances the version counters, and stays within the
measured ulp distance of torch.optim.Adam on the device."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# Packed back to back: offsets 0, 1, 4, 8, 13, 14, 1037, 2061, 3086, 7183 - odd, = 2 (mod 4) and = 0 (mod 4); tensors smaller than a
# vector; a tensor of several blocks (64*64*9 = 18 blocks of 2048) and partial last blocks (4097 = 2 blocks + 1 element).
SIZES = [1, 3, 4, 5, 1, 1023, 1024, 1025, 4097, 64 * 64 * 9]
# The same tensors in reverse order put the multi-block tensor and the 4097 one on offsets = 0 (mod 4): the 16-byte path over whole
# blocks, a partial block and a scalar tail (in SIZES only the tensors of 1, 4 and 5 elements take it).
LAYOUTS = {"issue": SIZES, "reversed": SIZES[::-1]}
GUARD = 12345.678
LR = 1e-4


def _weights(rs, n):
    """0.5 <= |p| < 2 with random signs (the scale at which an ulp of the weight is far above an ulp of the update, see
    test_resume_cpu.test_adam_step_host_is_torch_adam_within_one_ulp)"""
    return (rs.uniform(0.5, 2.0, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)


def _gradients(rs, n):
    """magnitudes from 1e-25 to 10 (squares from 0 through the subnormals up to 100) with a tenth exact zeros"""
    g = rs.standard_normal(n) * 10.0 ** rs.uniform(-25.0, 1.0, n)
    g[rs.uniform(size=n) < 0.1] = 0.0
    g = g.astype(np.float32)
    g[:4] = [1e-20, -1e-20, 0.0, 10.0]                           # (1e-20)^2 (1 - b2) is a subnormal second moment
    return g


def _guarded(values: np.ndarray):
    """(view of the first len(values) elements, the 4 guard words behind them) of one device allocation"""
    store = torch.full((len(values) + 4,), GUARD, dtype=torch.float32, device="cuda")
    store[:len(values)] = torch.from_numpy(values).cuda()
    return store[:len(values)], store[len(values):]


def _setup(sizes, betas, wd, seed=0, zero_head=False):
    """zero_head: the first four weights (where `_gradients` puts +-1e-20, 0 and 10) are exact zeros, so that weight decay adds
    nothing to those gradients and their squares stay subnormal"""
    from fcvsr_amd.train import HipAdam
    rs = np.random.RandomState(seed)
    flat_p = _weights(rs, sum(sizes))
    if zero_head:
        flat_p[:4] = 0.0
    host_p = [a.copy() for a in np.split(flat_p, np.cumsum(sizes)[:-1])]
    params, guards = [], []
    for hp in host_p:
        view, guard = _guarded(hp)
        params.append(torch.nn.Parameter(view))
        guards.append(guard)
    names = [f"t{i}_{n}" for i, n in enumerate(sizes)]
    opt = HipAdam(params, names, lr=LR, betas=betas, eps=1e-8, weight_decay=wd)
    total = sum(sizes)
    zeros = np.zeros(total, np.float32)
    (opt.exp_avg, g1), (opt.exp_avg_sq, g2), (flat, g3) = _guarded(zeros), _guarded(zeros), _guarded(zeros)
    guards += [g1, g2, g3]
    return rs, host_p, params, opt, flat, guards


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("wd", [0.0, 1e-5])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.9, 0.99)])
def test_three_steps_equal_the_host_specification_bit_for_bit(betas, wd, layout):
    from fcvsr_amd.train.optim import adam_step_host
    sizes = LAYOUTS[layout]
    rs, host_p, params, opt, flat, guards = _setup(sizes, betas, wd, zero_head=True)
    assert {o % 4 for o in opt.offsets} == {0, 1, 2, 3}
    total = sum(sizes)
    p, m, v = np.concatenate(host_p), np.zeros(total, np.float32), np.zeros(total, np.float32)
    subnormal_seen = False
    for t in (1, 2, 3):
        g = _gradients(rs, total)
        flat.copy_(torch.from_numpy(g))
        versions = [q._version for q in params]
        opt.step(flat)
        torch.cuda.synchronize()
        p, m, v = adam_step_host(p, g, m, v, t, LR, betas, 1e-8, wd)
        subnormal_seen |= bool(((v > 0) & (v < np.finfo(np.float32).tiny)).any())
        assert opt.t == t
        got_p = torch.cat([q.detach().reshape(-1) for q in params]).cpu()
        for name, got, want in (("p", got_p, p), ("exp_avg", opt.exp_avg.cpu(), m), ("exp_avg_sq", opt.exp_avg_sq.cpu(), v)):
            want = torch.from_numpy(want)
            if not torch.equal(got, want):
                bad = torch.nonzero(got.view(torch.int32) != want.view(torch.int32)).flatten()
                i = int(bad[0])
                raise AssertionError(f"step {t}: {name} differs from adam_step_host in {len(bad)} of {total} elements, first at flat "
                                     f"index {i}: kernel {float(got[i])!r}, host {float(want[i])!r}, gradient {float(g[i])!r}")
        assert torch.equal(flat.cpu(), torch.from_numpy(g)), "the gradient buffer is read-only"
        assert all(q._version > before for q, before in zip(params, versions)), "every parameter's version counter advances"
        for gd in guards:
            assert torch.equal(gd.cpu(), torch.full((4,), GUARD)), "a guard word behind a buffer changed"
    assert subnormal_seen, "the gradients must put subnormal second moments on the path"


def test_ulp_distance_to_torch_adam_on_the_device():
    """Three chained steps of HipAdam against three of torch.optim.Adam(foreach=False) on the device, same weights and gradients
    (SIZES layout, betas (0.9, 0.99), weight decay 1e-5).  torch rounds lerp and addcdiv differently, so this is a distance, not an
    equality.  Measured on an MI355X: largest distance MEASURED_ULP = 1 ulp of the f32 parameter (see profiles/NOTES.md); asserted:
    at most twice that."""
    MEASURED_ULP = 1
    betas, wd = (0.9, 0.99), 1e-5
    rs, host_p, params, opt, flat, _ = _setup(SIZES, betas, wd)
    twins = [torch.nn.Parameter(torch.from_numpy(hp).cuda()) for hp in host_p]
    ref = torch.optim.Adam(twins, lr=LR, betas=betas, eps=1e-8, weight_decay=wd, foreach=False)
    total = sum(SIZES)
    for _ in range(3):
        g = torch.from_numpy(_gradients(rs, total)).cuda()
        flat.copy_(g)
        for q, gq in zip(twins, g.split(SIZES)):
            q.grad = gq.clone()
        opt.step(flat)
        ref.step()
    torch.cuda.synchronize()

    def line(x):
        i = x.detach().reshape(-1).cpu().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    worst = max(int((line(a) - line(b)).abs().max()) for a, b in zip(params, twins))
    print(f"HipAdam vs torch.optim.Adam(foreach=False) after 3 steps: largest distance {worst} ulp")
    assert worst <= 2 * MEASURED_ULP


def test_bad_arguments_are_refused_before_any_launch():
    from fcvsr_amd import hip
    from fcvsr_amd.train import HipAdam
    L = hip.lib()
    assert L.fcvsr_adam_multi_block_elems() == 2048
    buf = torch.zeros(64, device="cuda")
    tab = torch.tensor([[buf.data_ptr(), 0, 16, 0]], dtype=torch.int64).cuda()
    scal = (0.001, 0.1, 0.1, 0.999, 0.001, 1e-8, 0.0)
    m, v, g = (torch.zeros(16, device="cuda") for _ in range(3))
    s = hip.stream_ptr()
    E_ARG = -1
    assert L.fcvsr_adam_multi(None, 1, 1, g.data_ptr(), m.data_ptr(), v.data_ptr(), 1, *scal, s) == E_ARG
    assert L.fcvsr_adam_multi(tab.data_ptr(), 1, 1, None, m.data_ptr(), v.data_ptr(), 1, *scal, s) == E_ARG
    assert L.fcvsr_adam_multi(tab.data_ptr(), 1, 1, g.data_ptr(), None, v.data_ptr(), 1, *scal, s) == E_ARG
    assert L.fcvsr_adam_multi(tab.data_ptr(), 1, 1, g.data_ptr(), m.data_ptr(), None, 1, *scal, s) == E_ARG
    assert L.fcvsr_adam_multi(tab.data_ptr(), 0, 0, g.data_ptr(), m.data_ptr(), v.data_ptr(), 1, *scal, s) == E_ARG
    assert L.fcvsr_adam_multi(tab.data_ptr(), 1, 1, g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, *scal, s) == E_ARG
    assert b"step count" in L.fcvsr_last_error()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0 and float(m.abs().sum()) == 0.0
    p = torch.nn.Parameter(torch.ones(8, device="cuda"))
    opt = HipAdam([p], ["p"], lr=1e-3)
    with pytest.raises(ValueError, match="flat float32 gradient"):
        opt.step(torch.zeros(9, device="cuda"))
    with pytest.raises(ValueError, match="one distinct name"):
        HipAdam([p], ["p", "q"], lr=1e-3)
    with pytest.raises(ValueError, match="empty"):
        HipAdam([], [], lr=1e-3)
