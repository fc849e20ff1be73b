"""The compiled Gaussian adapter's intrinsics gradient: gsr_adapt_backward_ex (the second instance of the backward kernel, the
22-float partial rows and the camera reduce) behind GaussianAdapter(fused=True) with intrinsics that require grad.

Checker: the one tests/test_adapter_hip.py uses - GaussianAdapter's torch ops in float64 on the CPU (pinned to the reference's
recorded outputs by tests/test_adapter.py).  Bar: the project's rel-L2 < 1e-4 for HIP against its checker, over the tensor and for each
group on its own; the closed form of the chain back to K is held to 1e-12 in float64 without a GPU.  The float32 torch path's own
distance from float64 is printed next to every HIP figure (docs/PARITY.md quotes them)."""
import os

import numpy as np
import pytest
import torch

import pf3plat_amd
from pf3plat_amd import _lib
from pf3plat_amd.adapter import GaussianAdapter, GaussianAdapterCfg
from tests import test_adapter_hip as base
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = base.NAMES
GRADS = ("d_raw", "d_depths", "d_coordinates", "d_extrinsics")
LO, HI = 0.5, 15.0


def _general_intrinsics(b, v, seed):
    """(b, v, 1, 3, 3), a different K per group: focal lengths 0.6-1.2, principal point off-centre, skew of a few 1e-2 (a smaller
    entry below the diagonal as well), bottom row perturbed by a few 1e-3 - all nine entries matter and no two groups are alike."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand((b, v), generator=g)
    sign = lambda: torch.where(torch.rand((b, v), generator=g) < 0.5, -1.0, 1.0)
    k = torch.zeros(b, v, 3, 3)
    k[..., 0, 0], k[..., 1, 1] = u(0.6, 1.2), u(0.6, 1.2)
    k[..., 0, 2], k[..., 1, 2] = 0.5 + sign() * u(0.03, 0.1), 0.5 + sign() * u(0.03, 0.1)
    k[..., 0, 1], k[..., 1, 0] = sign() * u(0.01, 0.05), sign() * u(0.005, 0.02)
    k[..., 2, 0], k[..., 2, 1], k[..., 2, 2] = sign() * u(0.001, 0.005), sign() * u(0.001, 0.005), 1.0 + sign() * u(0.001, 0.005)
    return k[:, :, None]


def _case(p, degree, seed, b=2, v=2):
    ext, _, _, _ = base._sources(b, v, 1, 1, seed=seed)
    g = torch.Generator().manual_seed(1000 * degree + seed)
    m = (degree + 1) ** 2
    coords = torch.rand((b, v, p, 2), generator=g)
    depths = 1.0 + 4.0 * torch.rand((b, v, p), generator=g)
    raw = torch.randn((b, v, p, 7 + 3 * m), generator=g)
    cots = [torch.randn((b, v, p, *tail), generator=g) for tail in ((3,), (3,), (4,), (3, m))]
    return ext, _general_intrinsics(b, v, seed + 1), coords, depths, raw, cots


def _run(ad, case, hw, dtype, device, intr_grad=True, twice=False):
    """Forward + backward of one adapter on copies of the inputs in (dtype, device) -> outputs, gradients (raw, depths, coordinates,
    extrinsics and - with intr_grad - the (b, v, 1, 3, 3) intrinsics leaf), and those of a second backward over the retained graph if `twice`."""
    ext, intr, coords, depths, raw, cots = case
    mk = lambda x, grad=True: x.detach().to(device=device, dtype=dtype).clone().requires_grad_(grad)
    e, c, d, r, k = mk(ext), mk(coords), mk(depths), mk(raw), mk(intr, intr_grad)
    opac = torch.ones(depths.shape, dtype=dtype, device=device)
    out = ad.to(device).forward(e, k, c, d, opac, r, hw)
    outs = [getattr(out, n) for n in NAMES]
    loss = sum((o * ct.to(device=device, dtype=dtype)).sum() for o, ct in zip(outs, cots))
    leaves = (r, d, c, e) + ((k,) if intr_grad else ())
    g1 = torch.autograd.grad(loss, leaves, retain_graph=twice)
    g2 = torch.autograd.grad(loss, leaves) if twice else None
    return [o.detach() for o in outs], g1, g2


def _closed_form(ext, intr, coords, depths, raw, cots, hw):
    """dL/dintrinsics the way the kernels form it, restated in torch (any dtype): per group the sums Ginv = sum d_p (x) (u, v, 1) and
    g_mult = sum depth x sum_r dscale[r] (lo + (hi - lo) sigmoid(r)), then dL/dK = -K^-T Ginv K^-T and
    dL/dK[:2, :2] += -0.1 g_mult (K2^-T 1) (K2^-1 q)^T."""
    h, w = hw
    b, v, p = depths.shape
    K, R = intr.reshape(b * v, 3, 3), ext.reshape(b * v, 4, 4)[:, :3, :3]
    x = torch.cat((coords, torch.ones_like(coords[..., :1])), -1).reshape(b * v, p, 3)
    dep = depths.reshape(b * v, p)
    gm, gs = cots[0].reshape(b * v, p, 3), cots[1].reshape(b * v, p, 3)
    kinv = torch.linalg.inv(K)
    pt = x @ kinv.transpose(1, 2)
    n = pt.norm(dim=-1, keepdim=True)
    ray = pt / n
    d_ray = (gm * dep[..., None]) @ R  # d_ray[c] = sum_r R[r][c] dmean[r] depth
    d_p = (d_ray - ray * (ray * d_ray).sum(-1, keepdim=True)) / n
    ginv = d_p.transpose(1, 2) @ x
    sig = torch.sigmoid(raw.reshape(b * v, p, -1)[..., :3])
    g_mult = (dep * (gs * (LO + (HI - LO) * sig)).sum(-1)).sum(-1)
    d_k = -kinv.transpose(1, 2) @ ginv @ kinv.transpose(1, 2)
    k2inv = torch.linalg.inv(K[:, :2, :2])
    q = torch.tensor((1.0 / w, 1.0 / h), dtype=K.dtype)
    ones = k2inv.transpose(1, 2) @ torch.ones(2, dtype=K.dtype)
    foot = -0.1 * g_mult[:, None, None] * ones[:, :, None] * (k2inv @ q)[:, None, :]
    d_k[:, :2, :2] = d_k[:, :2, :2] + foot
    return d_k.reshape(intr.shape)


# ---- without a GPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_extended_adapter_entry_points():
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in ("gsr_adapt_backward_ex", "gsr_adapt_partials_bytes_ex"):
        assert f"{name}(" in header and name in _lib.EXPORTED_SYMBOLS
        getattr(lib, name)
    assert "#define GSR_ABI_VERSION 5" in header and lib.gsr_abi_version() == 5


def test_extended_partials_size_is_host_arithmetic():
    lib = _lib.load()
    for g, p in ((1, 1), (1, 64), (1, 65), (4, 1473), (8, 65536), (3, 1000)):
        plain = lib.gsr_adapt_partials_bytes(g, p)
        assert plain > 0 and lib.gsr_adapt_partials_bytes_ex(g, p, 0) == plain
        assert lib.gsr_adapt_partials_bytes_ex(g, p, 1) * 12 == plain * 22
    for g, p in ((0, 100), (3, 0), (-1, 5), (5, -1)):
        assert lib.gsr_adapt_partials_bytes_ex(g, p, 0) == 0 and lib.gsr_adapt_partials_bytes_ex(g, p, 1) == 0


def _ex_args(g=2, p=5, degree=4, stride=82, h=16, w=16, ptr=8, d_intr=8):
    """Arguments of gsr_adapt_backward_ex with every pointer the same non-NULL dummy: only calls that must return before any launch."""
    return [g, p, degree, ptr, ptr, ptr, ptr, ptr, stride, 0.5, 15.0, h, w, 1e-8] + [None] * 3 + [ptr] * 4 + [d_intr, ptr, None]


def test_extended_backward_rejects_bad_arguments_and_accepts_zero_gaussians():
    fn = _lib.load().gsr_adapt_backward_ex
    for d_intr in (8, None):
        for bad in (dict(g=-1), dict(p=-1), dict(degree=-1), dict(degree=5), dict(stride=81), dict(degree=2, stride=33), dict(h=0), dict(w=-4)):
            assert fn(*_ex_args(d_intr=d_intr, **bad)) == -1, (bad, d_intr)
        for k in (3, 4, 5, 6, 7, 17, 18, 19, 20, 22):  # every required pointer (the cotangents, 14-16, and dL_dintrinsics, 21, may be NULL)
            a = _ex_args(d_intr=d_intr)
            a[k] = None
            assert fn(*a) == -1, (k, d_intr)
        for zero in (dict(g=0), dict(p=0)):  # nothing to do: returns before it looks at a pointer
            assert fn(*_ex_args(ptr=None, d_intr=d_intr, **zero)) == 0, (zero, d_intr)


def test_closed_form_of_the_intrinsics_gradient_against_float64_autograd():
    """The two lines of the chain (include/gsr.h), restated in float64, against autograd of the torch adapter: general K, 2 x 2 groups."""
    hw = (24, 32)
    for degree, p in ((0, 130), (4, 37)):
        case = tuple(x.double() if torch.is_tensor(x) else [c.double() for c in x] for x in _case(p, degree, seed=5))
        _, grads, _ = _run(GaussianAdapter(GaussianAdapterCfg(LO, HI, degree), rotate_sh=None), case, hw, torch.float64, "cpu")
        want = grads[4].numpy()
        got = _closed_form(*case, hw).numpy()
        assert np.abs(want).max() > 0
        err = rel_l2(got, want)
        print(f"[adapter intrinsics] closed form vs float64 autograd, degree {degree} P {p}: {err:.3e}")
        assert err < 1e-12


# ---- on the MI355X ------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
HW = (24, 32)


def _intr_errors(tag, got, want, own=None):
    """rel-L2 of an intrinsics gradient against float64 over the tensor and for each group on its own, printed, the worst returned."""
    a, r = got.double().cpu().numpy(), want.cpu().numpy()
    assert np.isfinite(a).all(), tag
    groups = a.reshape(-1, 9).shape[0]
    errs = [rel_l2(a, r)] + [rel_l2(a.reshape(-1, 9)[i], r.reshape(-1, 9)[i]) for i in range(groups)]
    mine = ""
    if own is not None:
        o = own.double().cpu().numpy()
        mine = f"   float32 torch vs float64: {rel_l2(o, r):.3e} (worst group {max(rel_l2(o.reshape(-1, 9)[i], r.reshape(-1, 9)[i]) for i in range(groups)):.3e})"
    print(f"[adapter parity] {tag:28s} d_intrinsics   hip vs float64: {errs[0]:.3e} (worst group {max(errs[1:]):.3e}){mine}")
    return max(errs)


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [0, 4])
def test_intrinsics_gradient_at_edge_shapes(degree):
    """P of 1, 63, 65, 1000 and 1473 (1, 1, 2, 16 and 24 workgroup rows per group: fewer than the reduce's stride of 21, and more), a
    general K per group, random cotangents; dL/dintrinsics, in the leaf's (2, 2, 1, 3, 3) shape, against float64 on the CPU."""
    cfg = GaussianAdapterCfg(LO, HI, degree)
    for p in (1, 63, 65, 1000, 1473):
        case = _case(p, degree, seed=p)
        ad = GaussianAdapter(cfg, rotate_sh=None, fused=True)
        ho, hg, _ = _run(ad, case, HW, torch.float32, DEV)
        assert ad.last_path == "hip"
        assert hg[4].shape == (2, 2, 1, 3, 3)
        fo, fg, _ = _run(GaussianAdapter(cfg, rotate_sh=None), case, HW, torch.float32, DEV)
        ro, rg, _ = _run(GaussianAdapter(cfg, rotate_sh=None), case, HW, torch.float64, "cpu")
        assert float(rg[4].abs().min()) > 0  # all nine entries of every group are exercised
        base._compare(f"general K degree {degree} P {p}", ho + list(hg[:4]), ro + list(rg[:4]), fo + list(fg[:4]))
        assert _intr_errors(f"general K degree {degree} P {p}", hg[4], rg[4], fg[4]) < 1e-4


@pytest.mark.gpu
def test_nothing_else_moves_when_intrinsics_require_grad():
    cfg = GaussianAdapterCfg(LO, HI, 4)
    for p in (65, 1000):
        case = _case(p, 4, seed=p + 7)
        with_o, with_g, _ = _run(GaussianAdapter(cfg, rotate_sh=None, fused=True), case, HW, torch.float32, DEV)
        ad = GaussianAdapter(cfg, rotate_sh=None, fused=True)
        plain_o, plain_g, _ = _run(ad, case, HW, torch.float32, DEV, intr_grad=False)
        assert ad.last_path == "hip"
        for name, a, b in zip(NAMES + GRADS, with_o + list(with_g[:4]), plain_o + list(plain_g)):
            assert torch.equal(a, b), (p, name)


def _abi_case(gq=3, p=200, degree=2, stride=36, seed=11):
    m = (degree + 1) ** 2
    g = torch.Generator().manual_seed(seed)
    ext, _, _, _ = base._sources(1, gq, 1, 1)
    dev = lambda x: x.to(DEV).contiguous()
    ins = [dev(ext.reshape(gq, 4, 4)), dev(_general_intrinsics(1, gq, seed).reshape(gq, 3, 3)), dev(torch.rand((gq, p, 2), generator=g)),
           dev(1 + torch.rand((gq, p), generator=g)), dev(torch.randn((gq, p, stride), generator=g))]
    cots = [dev(torch.randn(s, generator=g)) for s in ((gq, p, 3), (gq, p, 7), (gq, p, 3, m))]
    return (gq, p, degree, stride, m), ins, cots


def _abi_backward(dims, ins, given, entry="ex", intrinsics=True):
    """One call through the C ABI on NaN-prefilled outputs -> [dL_draw, dL_ddepths, dL_dcoordinates, dL_dextrinsics(, dL_dintrinsics)]."""
    lib = _lib.load()
    gq, p, degree, stride, m = dims
    outs = [torch.full(s, float("nan"), device=DEV) for s in ((gq, p, 7 + 3 * m), (gq, p), (gq, p, 2), (gq, 4, 4))]
    head = [gq, p, degree, *[x.data_ptr() for x in ins], stride, LO, HI, 24, 32, 1e-8, *[None if c is None else c.data_ptr() for c in given],
            *[o.data_ptr() for o in outs]]
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "plain":
        partials = torch.empty(lib.gsr_adapt_partials_bytes(gq, p), dtype=torch.uint8, device=DEV)
        rc = lib.gsr_adapt_backward(*head, partials.data_ptr(), stream)
    else:
        partials = torch.empty(lib.gsr_adapt_partials_bytes_ex(gq, p, int(intrinsics)), dtype=torch.uint8, device=DEV)
        if intrinsics:
            outs.append(torch.full((gq, 3, 3), float("nan"), device=DEV))
        rc = lib.gsr_adapt_backward_ex(*head, outs[4].data_ptr() if intrinsics else None, partials.data_ptr(), stream)
    assert rc == 0
    torch.cuda.synchronize()
    return outs


@pytest.mark.gpu
def test_extended_backward_keeps_the_plain_call_s_bits_through_the_c_abi():
    dims, ins, cots = _abi_case()
    plain = _abi_backward(dims, ins, cots, entry="plain")
    null = _abi_backward(dims, ins, cots, intrinsics=False)
    full = _abi_backward(dims, ins, cots)
    assert len(null) == 4 and len(full) == 5
    for name, a, b, c in zip(GRADS, plain, null, full):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name  # NULL dL_dintrinsics: gsr_adapt_backward itself
        assert torch.equal(a, c), name  # non-NULL: the four old outputs do not move
    assert torch.isfinite(full[4]).all() and float(full[4].abs().min()) > 0


@pytest.mark.gpu
def test_two_backwards_give_the_same_intrinsics_gradient_bits():
    case = _case(1473, 4, seed=21)
    ad = GaussianAdapter(GaussianAdapterCfg(LO, HI, 4), rotate_sh=None, fused=True)
    _, g1, g2 = _run(ad, case, HW, torch.float32, DEV, twice=True)
    assert ad.last_path == "hip" and float(g1[4].abs().max()) > 0
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_zero_and_null_cotangents_with_an_intrinsics_gradient():
    dims, ins, cots = _abi_case()
    only_harmonics = _abi_backward(dims, ins, [None, None, cots[2]])
    assert torch.equal(only_harmonics[4], torch.zeros_like(only_harmonics[4]))  # fully written (NaN before), exactly zero
    assert float(only_harmonics[0].abs().max()) > 0
    for mask in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        got = _abi_backward(dims, ins, [c if on else None for c, on in zip(cots, mask)])
        want = _abi_backward(dims, ins, [c if on else torch.zeros_like(c) for c, on in zip(cots, mask)])
        for a, b in zip(got, want):
            assert torch.isfinite(a).all() and torch.equal(a, b), mask
    assert all(float(x.abs().max()) == 0.0 for x in _abi_backward(dims, ins, [None, None, None]))


@pytest.mark.gpu
def test_adapter_and_render_shares_of_the_intrinsics_gradient_add_up():
    """ONE intrinsics leaf feeds the adapter (as the source cameras) and the decoder (which renders the source views themselves):
    compiled adapter against torch adapter, the same decoder, both on the GPU; and the adapter's share alone is not zero."""
    b, v, hs, ws, hw = 1, 2, 32, 32, (32, 32)
    ext, intr, coords, depths = base._sources(b, v, hs, ws, seed=7)
    g = torch.Generator().manual_seed(8)
    wide = torch.randn((b, v, hs * ws, 84), generator=g).to(DEV)
    opac = (0.1 + 0.85 * torch.rand((b, v, hs * ws), generator=g)).to(DEV)
    near, far = torch.full((b, v), 0.5, device=DEV), torch.full((b, v), 20.0, device=DEV)
    w = torch.rand((b, v, 3, *hw), generator=g).to(DEV)
    wd = (0.05 * torch.rand((b, v, *hw), generator=g)).to(DEV)
    cfg = GaussianAdapterCfg(LO, HI, 4)
    dec = pf3plat_amd.DecoderSplattingCUDA().to(DEV)
    e = ext.reshape(b, v, 4, 4).to(DEV)

    def leaf_grad(fused, render_share):
        leaf = intr.reshape(b, v, 3, 3).to(DEV).clone().requires_grad_(True)
        ad = GaussianAdapter(cfg, fuse_sh_rotation=True, fused=fused).to(DEV)
        out = ad.forward(e[:, :, None], leaf[:, :, None], coords.to(DEV), depths.to(DEV), opac, wide[..., 2:], hw)
        assert ad.last_path == ("hip" if fused else "torch") and out.sh_frame == "e3nn"
        o = dec.forward(out.for_decoder(), e, leaf, near, far, hw, depth_mode="depth", intrinsics_gradients=render_share)
        ((o.color * w).sum() + (o.depth * wd).sum()).backward()
        return leaf.grad

    hip, ref = leaf_grad(True, True), leaf_grad(False, True)
    assert hip.shape == (b, v, 3, 3)
    err = rel_l2(hip.double().cpu().numpy(), ref.double().cpu().numpy())
    print(f"[adapter parity] end to end d_intrinsics (adapter + render) hip adapter vs torch adapter: {err:.3e}")
    assert float(ref.abs().max()) > 0 and err < 1e-4
    share, share_ref = leaf_grad(True, False), leaf_grad(False, False)  # the render's share off: what is left came through the adapter
    assert share is not None and float(share.abs().max()) > 0
    err = rel_l2(share.double().cpu().numpy(), share_ref.double().cpu().numpy())
    print(f"[adapter parity] end to end d_intrinsics (adapter's share alone, max |.| {float(share.abs().max()):.3e} of {float(hip.abs().max()):.3e}) "
          f"hip adapter vs torch adapter: {err:.3e}")
    assert err < 1e-4
