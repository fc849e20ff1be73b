"""The compiled Gaussian adapter: gsr_adapt / gsr_adapt_backward (one HIP launch each way) behind GaussianAdapter(fused=True).

Checker: the torch adapter (pf3plat_amd/adapter.py's torch ops, themselves pinned to the reference's recorded outputs by
tests/test_adapter.py) evaluated in float64 on the CPU, and tests/golden/adapter_fixtures.npz directly.  Bars: the fixture
tolerances test_adapter.py uses for the torch path (rtol 2e-5, atol 2e-7) and the project's rel-L2 < 1e-4 for HIP against its
checker.  The float32 torch path's own distance from float64 is printed next to every HIP figure (docs/PARITY.md quotes them)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import pf3plat_amd
from pf3plat_amd import _lib, splatting, synthetic
from pf3plat_amd.adapter import GaussianAdapter, GaussianAdapterCfg
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "adapter_fixtures.npz"))
t = lambda k: torch.tensor(FIX[k])
NAMES = ("means", "scales", "rotations", "harmonics")


# ---- without a GPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_adapter_entry_points():
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in ("gsr_adapt", "gsr_adapt_backward", "gsr_adapt_partials_bytes"):
        assert f"{name}(" in header and name in _lib.EXPORTED_SYMBOLS
        getattr(lib, name)
    assert "#define GSR_ABI_VERSION 5" in header and lib.gsr_abi_version() == 5


def _abi_args(g=2, p=5, degree=4, stride=82, h=16, w=16, ptr=8):
    """Argument lists of the two calls with every pointer the same non-NULL dummy: only calls that must return before any launch."""
    head = [g, p, degree, ptr, ptr, ptr, ptr, ptr, stride, 0.5, 15.0, h, w, 1e-8]
    return head + [ptr] * 3 + [None], head + [None] * 3 + [ptr] * 5 + [None]


def test_adapter_entry_points_reject_bad_arguments_and_accept_zero_gaussians():
    lib = _lib.load()
    calls = (lib.gsr_adapt, lib.gsr_adapt_backward)
    for bad in (dict(g=-1), dict(p=-1), dict(degree=-1), dict(degree=5), dict(stride=81), dict(degree=2, stride=33), dict(h=0), dict(w=-4)):
        for fn, args in zip(calls, _abi_args(**bad)):
            assert fn(*args) == -1, (fn.__name__, bad)
    fwd, bwd = _abi_args()
    for k in (3, 4, 5, 6, 7, 14, 15, 16):  # every required pointer of the forward
        a = list(fwd)
        a[k] = None
        assert lib.gsr_adapt(*a) == -1, k
    for k in (3, 4, 5, 6, 7, 17, 18, 19, 20, 21):  # ... of the backward (the three cotangents, 14-16, may be NULL)
        a = list(bwd)
        a[k] = None
        assert lib.gsr_adapt_backward(*a) == -1, k
    for zero in (dict(g=0), dict(p=0)):  # nothing to do: returns before it looks at a pointer
        for fn, args in zip(calls, _abi_args(ptr=None, **zero)):
            assert fn(*args) == 0, (fn.__name__, zero)


def test_adapter_partials_size_is_host_arithmetic():
    lib = _lib.load()
    assert lib.gsr_adapt_partials_bytes(0, 100) == 0 and lib.gsr_adapt_partials_bytes(3, 0) == 0 and lib.gsr_adapt_partials_bytes(-1, 5) == 0
    one = lib.gsr_adapt_partials_bytes(1, 1)
    assert one > 0 and one % 4 == 0
    assert lib.gsr_adapt_partials_bytes(8, 65536) == 8 * 1024 * one  # one row per 64-Gaussian workgroup
    assert lib.gsr_adapt_partials_bytes(1, 64) == one and lib.gsr_adapt_partials_bytes(1, 65) == 2 * one


def _fixture_call(ad, case="B", device="cpu"):
    hw = tuple(int(x) for x in FIX[case + "_hw"])
    mv = lambda k: t(k).to(device)
    pad = (slice(None), slice(None)) + (None,) * (FIX[case + "_in_opac"].ndim - 2)
    return ad.forward(mv(case + "_in_ext")[pad], mv(case + "_in_intr")[pad], mv(case + "_in_coords"), mv(case + "_in_depths"), mv(case + "_in_opac"),
                      mv(case + "_in_raw"), hw)


def _fixture_adapter(**kw):
    lo, hi, deg = FIX["B_cfg"]
    return GaussianAdapter(GaussianAdapterCfg(float(lo), float(hi), int(deg)), rotate_sh=None, **kw)


def test_fused_adapter_has_no_cpu_fallback_and_default_is_unchanged():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _fixture_call(_fixture_adapter(fused=True))
    ad = _fixture_adapter()
    assert ad.fused is False and ad.last_path is None
    out = _fixture_call(ad)
    assert ad.last_path == "torch"
    for name in NAMES:
        np.testing.assert_allclose(getattr(out, name).numpy(), FIX["B_out_" + name], rtol=2e-5, atol=2e-7, err_msg=name)
    # shapes the compiled path does not cover run the torch ops, also with fused=True (fixture case C: 2 surfaces x 2 samples)
    ad = _fixture_adapter(fused=True)
    out = _fixture_call(ad, "C")
    assert ad.last_path == "torch"
    np.testing.assert_allclose(out.means.numpy(), np.broadcast_to(FIX["C_out_means"], out.means.shape), rtol=2e-5, atol=2e-7)


def test_splatting_passes_one_record_tensor_on_and_concatenates_anything_else():
    rec = torch.randn(2, 3, 5, 7)
    s, r = rec[..., :3], rec[..., 3:]
    assert splatting._scale_rot_records(s, r).data_ptr() == rec.data_ptr()
    flat = splatting._scale_rot_records(s.reshape(2, 15, 3), r.reshape(2, 15, 4))  # for_decoder's reshapes are views
    assert flat.data_ptr() == rec.data_ptr() and flat.shape == (2, 15, 7) and torch.equal(flat, rec.reshape(2, 15, 7))
    for a, b in ((s.clone(), r.clone()), (s, r.clone()), (s[:1], r[:1]), (s[:, :, ::2], r[:, :, ::2]), (rec[..., 1:4], rec[..., 3:]),
                 (torch.randn(2, 6, 8)[..., :3], torch.randn(2, 6, 8)[..., 4:])):
        got = splatting._scale_rot_records(a, b)
        assert got.data_ptr() != rec.data_ptr() and torch.equal(got, torch.cat((a, b), -1))


# ---- on the MI355X ------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


@pytest.mark.gpu
def test_fixture_cases_through_the_compiled_path():
    ad = _fixture_adapter(fused=True).to(DEV)
    out = _fixture_call(ad, "B", DEV)
    assert ad.last_path == "hip"
    for name in NAMES:
        np.testing.assert_allclose(getattr(out, name).cpu().numpy(), FIX["B_out_" + name], rtol=2e-5, atol=2e-7, err_msg=name)
    assert out.scales._base is out.rotations._base and out.scales._base is not None
    out = _fixture_call(ad, "C", DEV)
    assert ad.last_path == "torch"
    for name in NAMES:
        got = getattr(out, name).cpu().numpy()
        np.testing.assert_allclose(got, np.broadcast_to(FIX["C_out_" + name], got.shape), rtol=2e-5, atol=2e-7, err_msg=name)


def _sources(b, v, hs, ws, seed=3):
    """Source cameras and per-pixel maps in the manner of tools/adapter_step.py: a few degrees of rotation per view, a wavy depth map."""
    g = torch.Generator().manual_seed(seed)
    ext = torch.eye(4).repeat(b, v, 1, 1)
    for i in range(b):
        for j in range(v):
            a = 0.1 * (torch.rand(3, generator=g) - 0.5)
            k = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            ext[i, j, :3, :3] = torch.linalg.matrix_exp(k)
            ext[i, j, 0, 3] = -0.5 + j / max(v - 1, 1)
    intr = torch.tensor([[0.86, 0, 0.5], [0, 0.86, 0.5], [0, 0, 1]]).repeat(b, v, 1, 1)
    yy, xx = torch.meshgrid((torch.arange(hs) + 0.5) / hs, (torch.arange(ws) + 0.5) / ws, indexing="ij")
    coords = torch.stack((xx, yy), -1).reshape(1, 1, hs * ws, 2).expand(b, v, hs * ws, 2).contiguous()
    depths = 3.0 + torch.sin(6 * xx + 2 * yy).reshape(1, 1, hs * ws) + 0.02 * torch.rand((b, v, hs * ws), generator=g)
    return ext[:, :, None], intr[:, :, None], coords, depths


def _grad_run(ad, ext, intr, coords, depths, raw_of, wide, hw, cots, dtype, device, twice=False):
    """Forward + backward of one adapter on copies of the inputs in (dtype, device); raw = raw_of(leaf made from `wide`).
    -> outputs, gradients (raw's leaf, depths, coordinates, extrinsics), and the gradients of a second backward if `twice`."""
    mk = lambda x, grad=True: x.detach().to(device=device, dtype=dtype).clone().requires_grad_(grad)
    e, c, d, wl = mk(ext), mk(coords), mk(depths), mk(wide)
    k = mk(intr, False)
    opac = torch.ones(depths.shape, dtype=dtype, device=device)
    out = ad.forward(e, k, c, d, opac, raw_of(wl), hw)
    outs = [getattr(out, n) for n in NAMES]
    loss = sum((o * ct.to(device=device, dtype=dtype)).sum() for o, ct in zip(outs, cots))
    leaves = (wl, d, c, e)
    g1 = torch.autograd.grad(loss, leaves, retain_graph=twice)
    g2 = torch.autograd.grad(loss, leaves) if twice else None
    return [o.detach() for o in outs], g1, g2


def _compare(tag, hip, ref64, f32=None, bar=1e-4, names=NAMES + ("d_raw", "d_depths", "d_coordinates", "d_extrinsics")):
    worst = {}
    for k, name in enumerate(names):
        a, r = hip[k].double().cpu().numpy(), ref64[k].cpu().numpy()
        assert np.isfinite(a).all(), (tag, name)
        worst[name] = rel_l2(a, r)
        own = "" if f32 is None else f"   float32 torch vs float64: {rel_l2(f32[k].double().cpu().numpy(), r):.3e}"
        print(f"[adapter parity] {tag:28s} {name:14s} hip vs float64: {worst[name]:.3e}{own}")
    for name, v in worst.items():
        assert v < bar, (tag, name, v)
    return worst


@pytest.mark.gpu
def test_forward_and_backward_at_pf3plats_training_shape():
    """4 scenes x 2 source views x 256 x 256 Gaussians, degree 4 (the inputs of tools/adapter_step.py), raw handed over as the
    [..., 2:] slice of an 84-wide tensor and read in place; every output and every gradient against float64 on the CPU."""
    spec = importlib.util.spec_from_file_location("adapter_step", os.path.join(ROOT, "tools", "adapter_step.py"))
    step = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(step)
    (ext, intr, coords, depths, _, raw, _, _), _ = step.inputs("cpu")
    hw = step.HW
    wide = torch.cat((torch.randn((*raw.shape[:-1], 2), generator=torch.Generator().manual_seed(1)), raw), -1)
    g = torch.Generator().manual_seed(2)
    cots = [torch.randn((*depths.shape, *tail), generator=g) for tail in ((3,), (3,), (4,), (3, 25))]
    cfg = GaussianAdapterCfg(0.5, 15.0, 4)
    tail = lambda x: x[..., 2:]
    hip_ad = GaussianAdapter(cfg, rotate_sh=None, fused=True)
    ho, hg, hg2 = _grad_run(hip_ad, ext, intr, coords, depths, tail, wide, hw, cots, torch.float32, DEV, twice=True)
    assert hip_ad.last_path == "hip"
    for a, b in zip(hg, hg2):  # the same bits from a second backward, the fixed-order camera sum included
        assert torch.equal(a, b)
    assert torch.equal(hg[0][..., :2], torch.zeros_like(hg[0][..., :2]))  # the two columns in front of the slice get nothing
    torch_ad = GaussianAdapter(cfg, rotate_sh=None)
    fo, fg, _ = _grad_run(torch_ad.to(DEV), ext, intr, coords, depths, tail, wide, hw, cots, torch.float32, DEV)
    ro, rg, _ = _grad_run(GaussianAdapter(cfg, rotate_sh=None), ext, intr, coords, depths, tail, wide, hw, cots, torch.float64, "cpu")
    assert float(rg[3].abs().max()) > 0 and float(rg[2].abs().max()) > 0
    _compare("training shape 4x2x65536", ho + list(hg), ro + list(rg), fo + list(fg))


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4])
def test_edge_shapes_and_values(degree):
    """P of 1, 63, 192 and 1000 (none a multiple of a workgroup's 64), contiguous raw (row stride = row width), scale features of +-50
    (a saturated sigmoid) and one all-zero quaternion row: finite, and equal to torch in float64."""
    cfg = GaussianAdapterCfg(0.5, 15.0, degree)
    m = (degree + 1) ** 2
    for p in (1, 63, 192, 1000):
        ext, intr, _, _ = _sources(2, 2, 1, 1, seed=p)
        g = torch.Generator().manual_seed(100 * degree + p)
        coords = torch.rand((2, 2, p, 2), generator=g)
        depths = 1.0 + 4.0 * torch.rand((2, 2, p), generator=g)
        raw = torch.randn((2, 2, p, 7 + 3 * m), generator=g)
        raw[0, 0, 0, :3] = torch.tensor([50.0, -50.0, 50.0])
        raw[1, 1, p - 1, :3] = -50.0
        zero_row = (1, 0, p // 2)
        raw[zero_row][3:7] = 0.0
        cots = [torch.randn((2, 2, p, *tail), generator=g) for tail in ((3,), (3,), (4,), (3, m))]
        same = lambda x: x
        ad = GaussianAdapter(cfg, rotate_sh=None, fused=True)
        ho, hg, _ = _grad_run(ad, ext, intr, coords, depths, same, raw, (24, 32), cots, torch.float32, DEV)
        assert ad.last_path == "hip" and hg[0].shape == raw.shape
        ro, rg, _ = _grad_run(GaussianAdapter(cfg, rotate_sh=None), ext, intr, coords, depths, same, raw, (24, 32), cots, torch.float64, "cpu")
        assert float(ho[2][zero_row].abs().max()) == 0.0 and float(ro[2][zero_row].abs().max()) == 0.0
        _compare(f"degree {degree} P {p}", ho + list(hg), ro + list(rg))
        # the zero quaternion's gradient is cotangent / eps (1e8 times the others): the rest of dL/draw on its own
        keep = torch.ones(raw.shape[:-1], dtype=torch.bool)
        keep[zero_row] = False
        if p > 1:
            assert rel_l2(hg[0].cpu()[keep].double().numpy(), rg[0][keep].numpy()) < 1e-4
        np.testing.assert_allclose(hg[0].cpu()[zero_row][3:7].numpy(), (cots[2][zero_row] / 1e-8).numpy(), rtol=1e-5)


@pytest.mark.gpu
def test_null_cotangents_through_the_c_abi():
    """NULL dL_dmeans / dL_dscale_rot / dL_dharmonics mean zeros: each combination equals the call with explicit zero arrays."""
    lib = _lib.load()
    gq, p, degree, stride = 3, 200, 2, 36  # rows of 34 floats, 36 apart
    m = (degree + 1) ** 2
    g = torch.Generator().manual_seed(11)
    ext, intr, _, _ = _sources(1, gq, 1, 1)
    dev = lambda x: x.to(DEV).contiguous()
    ext, intr = dev(ext.reshape(gq, 4, 4)), dev(intr.reshape(gq, 3, 3))
    coords, depths = dev(torch.rand((gq, p, 2), generator=g)), dev(1 + torch.rand((gq, p), generator=g))
    raw = dev(torch.randn((gq, p, stride), generator=g))
    cots = [dev(torch.randn(s, generator=g)) for s in ((gq, p, 3), (gq, p, 7), (gq, p, 3, m))]
    partials = torch.empty(lib.gsr_adapt_partials_bytes(gq, p), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def backward(given):
        outs = [torch.full(s, float("nan"), device=DEV) for s in ((gq, p, 7 + 3 * m), (gq, p), (gq, p, 2), (gq, 4, 4))]
        rc = lib.gsr_adapt_backward(gq, p, degree, ext.data_ptr(), intr.data_ptr(), coords.data_ptr(), depths.data_ptr(), raw.data_ptr(), stride, 0.5, 15.0,
                                    24, 32, 1e-8, *[None if c is None else c.data_ptr() for c in given], *[o.data_ptr() for o in outs],
                                    partials.data_ptr(), stream)
        assert rc == 0
        torch.cuda.synchronize()
        return outs

    for mask in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        got = backward([c if on else None for c, on in zip(cots, mask)])
        want = backward([c if on else torch.zeros_like(c) for c, on in zip(cots, mask)])
        for a, b in zip(got, want):
            assert torch.isfinite(a).all() and torch.equal(a, b), mask
    assert all(float(x.abs().max()) == 0.0 for x in backward([None, None, None]))


@pytest.mark.gpu
def test_fused_adapter_into_the_decoder_end_to_end(monkeypatch):
    """Compiled adapter (harmonics left in their frame) -> DecoderSplattingCUDA -> loss -> backward against the torch adapter ->
    the same decoder, both on the GPU; the decoder receives the adapter's record tensor itself, not a concatenated copy."""
    b, v, hs, ws, hw = 1, 2, 32, 32, (32, 32)
    ext, intr, coords, depths = _sources(b, v, hs, ws, seed=7)
    g = torch.Generator().manual_seed(8)
    wide = torch.randn((b, v, hs * ws, 84), generator=g)
    opac = (0.1 + 0.85 * torch.rand((b, v, hs * ws), generator=g)).to(DEV)
    sc = synthetic.make_scene(50, 8, hw, num_views=2)  # (only its cameras are used)
    cams = [x.to(DEV) for x in (sc.extrinsics, sc.intrinsics, sc.near, sc.far)]
    w = torch.rand((b, 2, 3, *hw), generator=g).to(DEV)
    wd = (0.05 * torch.rand((b, 2, *hw), generator=g)).to(DEV)
    cfg = GaussianAdapterCfg(0.5, 15.0, 4)
    dec = pf3plat_amd.DecoderSplattingCUDA().to(DEV)
    seen = []
    real = splatting.rasterize_views
    monkeypatch.setattr(splatting, "rasterize_views", lambda means, cov, *a, **k: (seen.append(cov), real(means, cov, *a, **k))[1])
    res = {}
    for name, ad in (("hip", GaussianAdapter(cfg, fuse_sh_rotation=True, fused=True)), ("torch", GaussianAdapter(cfg, fuse_sh_rotation=True))):
        mk = lambda x: x.detach().to(DEV).clone().requires_grad_(True)
        e, d, wl = mk(ext), mk(depths), mk(wide)
        out = ad.to(DEV).forward(e, intr.to(DEV), coords.to(DEV), d, opac, wl[..., 2:], hw)
        assert ad.last_path == name and out.sh_frame == "e3nn"
        o = dec.forward(out.for_decoder(), *cams, hw, depth_mode="depth")
        ((o.color * w).sum() + (o.depth * wd).sum()).backward()
        if name == "hip":
            assert seen[-1].data_ptr() == out.scales.data_ptr() and seen[-1]._base is out.scales._base and seen[-1].shape == (b, v * hs * ws, 7)
        else:
            assert seen[-1]._base is None  # (the torch adapter's two tensors are concatenated)
        res[name] = [x.detach().double().cpu().numpy() for x in (o.color, o.depth, wl.grad, d.grad, e.grad)]
    for k, what in enumerate(("colour", "depth", "d_raw", "d_depths", "d_extrinsics")):
        err = rel_l2(res["hip"][k], res["torch"][k])
        print(f"[adapter parity] end to end {what:14s} hip adapter vs torch adapter: {err:.3e}")
        assert np.abs(res["torch"][k]).max() > 0 and err < 1e-4, what
