"""Helpers for the `-m gpu` parity tests: run the HIP library through the product's operator surface and the
CPU oracle on the same inputs, and decode the library's workspaces for stage-level comparisons."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from oracle import adapter
from pf3plat_amd import _lib, rasterizer
from pf3plat_amd.rasterizer import RasterConfig, pack_views
from tests.oracle_backend import OracleBackend
from tests.util import make_camera


def viewbuf_from_cams(cams, bgs, scales=None, device="cpu"):
    v = len(cams)
    vm = torch.tensor(np.stack([c["viewmatrix"] for c in cams]).reshape(v, 4, 4), dtype=torch.float32)
    pm = torch.tensor(np.stack([c["projmatrix"] for c in cams]).reshape(v, 4, 4), dtype=torch.float32)
    cp = torch.tensor(np.stack([c["campos"] for c in cams]), dtype=torch.float32)
    tx = torch.tensor([c["tanfovx"] for c in cams], dtype=torch.float32)
    ty = torch.tensor([c["tanfovy"] for c in cams], dtype=torch.float32)
    bg = torch.tensor(np.asarray(bgs, dtype=np.float32).reshape(v, 3))
    sc = None if scales is None else torch.tensor(np.asarray(scales, dtype=np.float32))
    return pack_views(vm, pm, cp, tx, ty, bg, sc).to(device)


def decode_workspaces(backend, cfg: RasterConfig, saved):
    """-> dict of numpy arrays: geom (V,N,8 f32, word 7 = radius bits), depth (V,N) or None, ranges (V,T,2), point_list, keys, final_T, n_contrib, status."""
    dims, geom, binb, img = saved[:4]
    lay = backend.workspace_layout(dims)
    V, N, H, W = cfg.num_views, cfg.num_gaussians, cfg.height, cfg.width
    sgx, sgy = 2 * ((W + 15) // 16), 2 * ((H + 15) // 16)
    T = sgx * sgy
    gl = backend.geom_layout(dims)
    rb = gl["record_bytes"]  # 32: x, y, conic a b c, opacity, extra, radius bits
    g = geom[: V * N * rb].view(torch.float32).reshape(V, N, rb // 4).cpu().numpy()
    bits = geom[: V * N * rb].view(torch.int32).reshape(V, N, rb // 4)[:, :, 7].cpu().numpy()
    # depth: word 3 of the 16-byte footprint words, kept in memory only by the windowed binning chain
    depth = None if gl["aux"] < 0 else geom[gl["aux"]: gl["aux"] + V * N * 16].view(torch.float32).reshape(V, N, 4)[:, :, 3].cpu().numpy()
    o_rgbc = gl["rgbc"]
    rgbc = geom[o_rgbc: o_rgbc + V * N * 16].view(torch.float32).reshape(V, N, 4).cpu().numpy()
    cbits = geom[o_rgbc: o_rgbc + V * N * 16].view(torch.int32).reshape(V, N, 4)[:, :, 3].cpu().numpy()
    b = binb.cpu()
    st = b[:16]
    num_pairs = int(st[:8].view(torch.int64).item())
    ranges = b[lay["ranges"]: lay["ranges"] + V * T * 8].view(torch.int32).reshape(V, T, 2).numpy()
    walked = b[lay["tile_total"]: lay["tile_total"] + V * T * 4].view(torch.int32).reshape(V, T).numpy()  # list entries each tile's blend went through
    cap = int(dims.pair_capacity)
    plist = b[lay["point_list"]: lay["point_list"] + cap * 4].view(torch.int32).numpy()  # a tile's list: ranges[v, t]
    keys = b[lay["keys"]: lay["keys"] + cap * 8].view(torch.int64).numpy()
    im = img.cpu()
    final_T = im[lay["final_T"]: lay["final_T"] + V * H * W * 4].view(torch.float32).reshape(V, H, W).numpy()
    n_contrib = im[lay["n_contrib"]: lay["n_contrib"] + V * H * W * 4].view(torch.int32).reshape(V, H, W).numpy()
    return dict(geom=g, depth=depth, rgb=rgbc[:, :, :3], radius=bits & 0x0FFFFFFF, clamped=cbits & 7, ranges=ranges, walked=walked, point_list=plist, keys=keys,
                final_T=final_T, n_contrib=n_contrib, num_pairs=num_pairs, overflow=int(st[8:12].view(torch.int32).item()),
                max_list=int(st[12:16].view(torch.int32).item()), sgx=sgx, sgy=sgy, T=T)


SH_FRAME_BITS = {None: 0, "rasterizer": _lib.FLAG_SH_IN_FRAME, "e3nn": _lib.FLAG_SH_IN_FRAME | _lib.FLAG_SH_FRAME_E3NN}


def _with_sh_frame(cfg: RasterConfig, sh_frame):
    """cfg with the GSR_FLAG_SH_IN_FRAME bits of `sh_frame` (None, "rasterizer" or "e3nn") and without any others."""
    return dataclasses.replace(cfg, flags=(cfg.flags & ~SH_FRAME_BITS["e3nn"]) | SH_FRAME_BITS[sh_frame])


def cov6_in_kernel_order(records, frames=None):
    """(S, N, 7) scale + quaternion (x, y, z, w) records [+ (S, F, 3, 3) frames] -> (S, N, 6) fp32 covariances, in the kernels' operation
    order (gsr_common.h cov6_from_sr: Rq from the un-normalised quaternion, M = F Rq, Sigma = M diag(s^2) M^T; IEEE fp32, nothing
    contracted).  The oracle side of the scale / rotation form rasterizes these: both sides then project the same covariance bits - the
    conic of a thin Gaussian amplifies a one-ulp difference in its covariance by its condition number, past the 1e-5 of
    check_preprocess between two correct fp32 builds.  The formula itself is pinned to oracle/adapter.py's (fp64) by tests/test_sr_cases.py."""
    f = np.float32
    sr = records.detach().cpu().numpy().astype(np.float32)
    i, j, k, r = (sr[..., c] for c in range(3, 7))
    ts = f(2) / (i * i + j * j + k * k + r * r + f(1e-8))
    rq = [f(1) - ts * (j * j + k * k), ts * (i * j - k * r), ts * (i * k + j * r),
          ts * (i * j + k * r), f(1) - ts * (i * i + k * k), ts * (j * k - i * r),
          ts * (i * k - j * r), ts * (j * k + i * r), f(1) - ts * (i * i + j * j)]
    if frames is None:
        m = rq
    else:
        n, nf = sr.shape[1], frames.shape[1]
        fr = np.repeat(frames.detach().cpu().numpy().astype(np.float32), n // nf, axis=1) if n else np.zeros(sr.shape[:2] + (3, 3), np.float32)
        m = [fr[..., a, 0] * rq[b] + fr[..., a, 1] * rq[3 + b] + fr[..., a, 2] * rq[6 + b] for a in range(3) for b in range(3)]
    s0, s1, s2 = sr[..., 0] * sr[..., 0], sr[..., 1] * sr[..., 1], sr[..., 2] * sr[..., 2]

    def cov(a, b):
        return m[3 * a] * s0 * m[3 * b] + m[3 * a + 1] * s1 * m[3 * b + 1] + m[3 * a + 2] * s2 * m[3 * b + 2]

    return torch.from_numpy(np.stack([cov(0, 0), cov(0, 1), cov(0, 2), cov(1, 1), cov(1, 2), cov(2, 2)], -1).astype(np.float32))


def run_oracle(cfg: RasterConfig, viewbuf_cpu, means, cov6, opac, colors, extra=None, g_color=None, g_extra=None,
               oracle_dtype=np.float32, want_means2d=True, want_views=False, frames=None, sh_frame=None, threads=8):
    """The oracle side of `run_both`: -> dict(color, extra, radii, handles, stats[, grads]).  Scale / rotation form (cfg.scale_rot): the
    oracle rasterizes `cov6_in_kernel_order(records, frames)` and the records' gradient is pulled back through oracle/adapter.py's
    covariance in fp64.  sh_frame ("rasterizer" | "e3nn"): `colors` are in the coordinates of those frames - they
    are rotated to world space in fp64 (`rasterizer._rotate_in_frames`, the torch path GSR_FLAG_SH_IN_FRAME replaced), rendered, and the
    world harmonics' gradient is pulled back through that rotation with autograd: the gradient comes back in the frames' coordinates."""
    ob = OracleBackend(dtype=oracle_dtype, threads=threads)  # (threads=1: sums in one fixed order, the same figures on every run)
    cfg = _with_sh_frame(cfg, None)
    local = world = None
    colors_o = colors
    if sh_frame is not None:
        with torch.enable_grad():
            local = colors.detach().double().requires_grad_(True)
            world = rasterizer._rotate_in_frames(local, frames.double(), bool(cfg.flags & _lib.FLAG_SH_PLANAR), sh_frame)
        colors_o = world.detach().float().contiguous()
    cov_o = cov6
    if cfg.scale_rot:  # the covariance in the kernels' order; the records' gradient through oracle/adapter.py's formula in fp64 below
        cov_o = cov6_in_kernel_order(cov6, frames)
        cfg = dataclasses.replace(cfg, scale_rot=False)
    oc, oe, orad, osaved = ob.forward(cfg, viewbuf_cpu, means, cov_o, opac, colors_o, extra)
    out = dict(color=oc.numpy(), extra=None if oe is None else oe.numpy(), radii=orad.numpy(), handles=osaved, stats=ob.last_stats)
    if g_color is not None:
        og = list(ob.backward(cfg, osaved, viewbuf_cpu, means, cov_o, opac, colors_o, extra, g_color, g_extra, want_means2d,
                              want_views=want_views))
        if cov_o is not cov6:
            with torch.enable_grad():
                rec = cov6.detach().double().requires_grad_(True)
                graph = adapter.cov6_from_scale_rotation(rec, None if frames is None else frames.double())
            (d_rec,) = torch.autograd.grad(graph, rec, og[1].double())
            og[1] = d_rec.to(og[1].dtype)
        if world is not None:
            (d_local,) = torch.autograd.grad(world, local, og[3].double())
            og[3] = d_local.to(og[3].dtype)
        names = ("means", "cov6", "opac", "colors", "extra", "means2d", "views")
        out["grads"] = {n: (None if t is None else t.numpy()) for n, t in zip(names, og)}
    return out


def run_both(cfg: RasterConfig, viewbuf_cpu, means, cov6, opac, colors, extra=None, g_color=None, g_extra=None,
             oracle_dtype=np.float32, want_means2d=True, capacity=None, want_views=False, frames=None, sh_frame=None,
             rows_in_workspace=False):
    """Forward (+ backward if g_color is given) on the HIP backend and on the oracle.  Inputs are CPU torch tensors.
    frames / sh_frame (the scale / rotation form, cfg.scale_rot): the HIP side takes `frames` and the bits of `sh_frame` (added to
    cfg.flags); the oracle side is `run_oracle`.  rows_in_workspace: the backward accumulates into the rows a forward flagged
    GSR_FLAG_BACKWARD_FOLLOWS zero-filled (the training path)."""
    dev = torch.device("cuda:0")
    hip = rasterizer.HipBackend()
    args_cpu = (means, cov6, opac, colors, extra)
    args_gpu = tuple(None if a is None else a.to(dev).contiguous() for a in args_cpu)
    vb_gpu = viewbuf_cpu.to(dev)
    fr_gpu = None if frames is None else frames.to(dev)
    cfg_h = cfg if sh_frame is None else _with_sh_frame(cfg, sh_frame)
    hc, he, hr, hsaved = hip.forward(cfg_h, vb_gpu, *args_gpu, capacity=capacity, frames=fr_gpu)
    torch.cuda.synchronize()
    out = dict(hip=dict(color=hc.cpu().numpy(), extra=None if he is None else he.cpu().numpy(), radii=hr.cpu().numpy(),
                        ws=decode_workspaces(hip, cfg, hsaved), status=hip.last_status))
    if g_color is not None:
        hg = hip.backward(cfg_h, hsaved, vb_gpu, *args_gpu, g_color.to(dev), None if g_extra is None else g_extra.to(dev),
                          want_means2d, rows_in_workspace=rows_in_workspace, frames=fr_gpu, want_views=want_views)
        torch.cuda.synchronize()
        names = ("means", "cov6", "opac", "colors", "extra", "means2d", "views")
        out["hip"]["grads"] = {n: (None if t is None else t.cpu().numpy()) for n, t in zip(names, hg)}
    out["oracle"] = run_oracle(cfg, viewbuf_cpu, means, cov6, opac, colors, extra, g_color, g_extra, oracle_dtype, want_means2d,
                               want_views, frames, sh_frame)
    return out


def run_hip(cfg: RasterConfig, viewbuf_cpu, means, cov6, opac, colors, extra=None, g_color=None, g_extra=None, frames=None,
            sh_frame=None, want_views=False):
    """HIP backend only (cases the oracle has no defined answer for): -> dict(color, extra, radii, status[, grads]).  frames /
    sh_frame / want_views as in `run_both`."""
    dev = torch.device("cuda:0")
    hip = rasterizer.HipBackend()
    args_gpu = tuple(None if a is None else a.to(dev).contiguous() for a in (means, cov6, opac, colors, extra))
    vb_gpu = viewbuf_cpu.to(dev)
    fr_gpu = None if frames is None else frames.to(dev)
    cfg = cfg if sh_frame is None else _with_sh_frame(cfg, sh_frame)
    hc, he, hr, hsaved = hip.forward(cfg, vb_gpu, *args_gpu, frames=fr_gpu)
    torch.cuda.synchronize()
    out = dict(color=hc.cpu().numpy(), extra=None if he is None else he.cpu().numpy(), radii=hr.cpu().numpy(), status=hip.last_status)
    if g_color is not None:
        hg = hip.backward(cfg, hsaved, vb_gpu, *args_gpu, g_color.to(dev), None if g_extra is None else g_extra.to(dev), True,
                          frames=fr_gpu, want_views=want_views)
        torch.cuda.synchronize()
        names = ("means", "cov6", "opac", "colors", "extra", "means2d", "views")
        out["grads"] = {n: (None if t is None else t.cpu().numpy()) for n, t in zip(names, hg)}
    return out


def scene_tensors(scene, use_sh=True):
    from pf3plat_amd.synthetic import scene_operator_inputs

    return scene_operator_inputs(scene, use_sh)


def scene_viewbuf(scene, scale_invariant=True):
    """Camera records (V, 48) of a Scene as a CPU tensor, built by the oracle's camera arithmetic (oracle/cameras.py): both
    sides of a parity test render with exactly these records, so the raster path is what is compared (the device camera
    set-up has its own test against the same functions)."""
    s, v = scene.extrinsics.shape[:2]
    return OracleBackend().setup_views(scene.extrinsics.reshape(s * v, 4, 4), scene.intrinsics.reshape(s * v, 3, 3),
                                       scene.near.reshape(s * v), scene.far.reshape(s * v), scene.background.reshape(3),
                                       scale_invariant)
