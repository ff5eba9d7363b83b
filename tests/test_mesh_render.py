"""The mesh rasteriser (csrc/mesh_render.hip, diffmvs_amd/mesh_render.py) against a numpy fp64 / Python-int restatement of the contract
in include/dmvs.h at tolerance zero, and against geometry: a watertight lattice, an analytic plane, a sphere through TSDF fusion and back,
and a tree through the command line.  Every kernel test runs on the host emulation here and on the MI355X under -m gpu."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
from diffmvs_amd import _lib, formats as IO, mesh as M, mesh_render as MR, synth
from test_cloud_render import K0, files, rig, write_tree

H0, W0 = 37, 53
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
NEAR, FAR = 1.0, 1000.0


# ------------------------------------------------------------------------------------------ the contract, restated
def move(verts, T):
    """the optional transform: fp64 products and sums in the contract's order, one rounding to fp32"""
    verts = np.asarray(verts, np.float32)
    if T is None:
        return verts
    m, d = np.asarray(T, np.float64).reshape(-1, 4)[:3], verts.astype(np.float64)
    return np.stack([(((m[r, 0] * d[:, 0] + m[r, 1] * d[:, 1]) + m[r, 2] * d[:, 2]) + m[r, 3]).astype(np.float32) for r in range(3)], 1)


def setup(vm, tri, q, flags, H, W):
    """steps 1 to 8 for one (face, view) -> (slot, None) or (7, the snapped face)"""
    N = len(vm)
    if any(i < 0 or i >= N for i in tri):
        return 0, None
    P = vm[list(tri)].astype(np.float64)
    if not np.isfinite(P).all():
        return 0, None
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        x = ((q[0] * X + q[1] * Y) + q[2] * Z) + q[3]
        y = ((q[4] * X + q[5] * Y) + q[6] * Z) + q[7]
        z = ((q[16] * X + q[17] * Y) + q[18] * Z) + q[19]
        u, v = x / z, y / z
    if (z <= q[20]).any():
        return 1, None
    if (z > q[21]).all():
        return 2, None
    if not ((np.abs(u) <= 2.0 ** 20).all() and (np.abs(v) <= 2.0 ** 20).all()):
        return 3, None
    sx, sy = [int(s) for s in np.rint(u * 256.0)], [int(s) for s in np.rint(v * 256.0)]
    A = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sy[1] - sy[0]) * (sx[2] - sx[0])
    if A == 0:
        return 4, None
    if (flags & _lib.RASTER_CULL_NEG and A < 0) or (flags & _lib.RASTER_CULL_POS and A > 0):
        return 5, None
    order = [0, 1, 2]
    if A < 0:
        order, A = [0, 2, 1], -A
    sx, sy, z, ids = [sx[k] for k in order], [sy[k] for k in order], [float(z[k]) for k in order], [int(tri[k]) for k in order]
    c0, c1 = max(-((-min(sx)) // 256), 0), min(max(sx) // 256, W - 1)
    r0, r1 = max(-((-min(sy)) // 256), 0), min(max(sy) // 256, H - 1)
    if c0 > c1 or r0 > r1:
        return 6, None
    return 7, {"sx": sx, "sy": sy, "z": z, "A": A, "ids": ids, "box": (c0, c1, r0, r1)}


def pixels(ft, px, py):
    """steps 9 and 10 on int64 arrays px, py -> (covered, wq [3], zp)"""
    inside, e = np.ones(np.broadcast(px, py).shape, bool), []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        dx, dy = ft["sx"][b] - ft["sx"][a], ft["sy"][b] - ft["sy"][a]
        ek = dx * (256 * py - ft["sy"][a]) - dy * (256 * px - ft["sx"][a])
        inside &= (ek > 0) | ((ek == 0) & bool(dy > 0 or (dy == 0 and dx > 0)))
        e.append(ek)
    with np.errstate(all="ignore"):
        wq = [(e[k].astype(np.float64) / float(ft["A"])) * (1.0 / ft["z"][k]) for k in range(3)]
        zp = 1.0 / ((wq[0] + wq[1]) + wq[2])
    return inside, wq, zp


def restate(verts, faces, table, H, W, flags=0, T=None, vrgb=None):
    """-> zid uint64 [V,H,W], counts int64 [V,8], covered pixels, depth fp32, face int32, normal fp32 [V,H,W,3], rgb uint8 [V,H,W,3]"""
    vm, V = move(verts, T), len(table)
    zid, counts, covered = np.full((V, H, W), ALL, np.uint64), np.zeros((V, _lib.RASTER_SLOTS), np.int64), 0
    for v in range(V):
        for f, tri in enumerate(faces):
            slot, ft = setup(vm, tri, table[v], flags, H, W)
            counts[v, slot] += 1
            if ft is None:
                continue
            c0, c1, r0, r1 = ft["box"]
            inside, _, zp = pixels(ft, np.arange(c0, c1 + 1, dtype=np.int64)[None, :], np.arange(r0, r1 + 1, dtype=np.int64)[:, None])
            covered += int(inside.sum())
            key = (zp.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            win = zid[v, r0:r1 + 1, c0:c1 + 1]
            win[...] = np.minimum(win, np.where(inside & (zp <= table[v, 21]), key, ALL))
    hit = zid != ALL
    depth = np.where(hit, (zid >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0))
    face = np.where(hit, (zid & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    normal, rgb = np.zeros((V, H, W, 3), np.float32), np.zeros((V, H, W, 3), np.uint8)
    for v in range(V):
        E = table[v, 8:20].reshape(3, 4)
        for f in np.unique(face[v][hit[v]]):
            rows, cols = np.nonzero(face[v] == f)
            P = vm[list(faces[f])].astype(np.float64)
            a, b = P[1] - P[0], P[2] - P[0]
            c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
            ln = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
            if ln > 0 and np.isfinite(ln):
                n = c / ln
                nc = [(E[i, 0] * n[0] + E[i, 1] * n[1]) + E[i, 2] * n[2] for i in range(3)]
                pc = [((E[i, 0] * P[0, 0] + E[i, 1] * P[0, 1]) + E[i, 2] * P[0, 2]) + E[i, 3] for i in range(3)]
                if (nc[0] * pc[0] + nc[1] * pc[1]) + nc[2] * pc[2] > 0:
                    n = -n
                normal[v, rows, cols] = n.astype(np.float32)
            if vrgb is not None:
                slot, ft = setup(vm, faces[f], table[v], 0, H, W)
                inside, wq, zp = pixels(ft, cols.astype(np.int64), rows.astype(np.int64))
                assert slot == 7 and inside.all()
                col = vrgb[ft["ids"]].astype(np.float64)
                for i in range(3):
                    val = np.rint(((wq[0] * zp) * col[0, i] + (wq[1] * zp) * col[1, i]) + (wq[2] * zp) * col[2, i])
                    rgb[v, rows, cols, i] = np.minimum(np.maximum(val, 0.0), 255.0).astype(np.uint8)
    return zid, counts, covered, depth, face, normal, rgb


def dev(ops, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a).view(np.uint32)


def run(ops, verts, faces, table, H, W, cull=None, T=None, vrgb=None, **kw):
    v, f = dev(ops, np.asarray(verts, np.float32)), dev(ops, np.asarray(faces, np.int32))
    zid, counts, work = ops.mesh_raster_zid(v, f, table, (H, W), cull=cull, transform=T, work=True, **kw)
    depth, face, normal, rgb = ops.mesh_raster_resolve(zid, v, f, table, transform=T, vrgb=None if vrgb is None else dev(ops, vrgb), normals=True)
    return zid, counts, work, depth, face, normal, rgb


# ------------------------------------------------------------------------------------------ 1. restatement, tolerance zero
TRANSFORM = np.array([[0.0, -1.0, 0.0, 16.0], [1.0, 0.0, 0.0, -8.0], [0.0, 0.0, 1.25, -40.0]])      # a quarter turn, a stretch, a shift


@pytest.fixture(scope="module")
def exact_case():
    """V = 9 (two view chunks), 37 x 53, 200 random faces of about 5 to 25 pixels in a slab that spills over every border and over
    `far`, plus the planted ones.  View 1 of rig(9) is the identity: u = 60 X / Z + 26, v = 60 Y / Z + 18."""
    rs = np.random.RandomState(5)
    centre = np.stack([rs.uniform(-420.0, 420.0, 200), rs.uniform(-300.0, 300.0, 200), rs.uniform(300.0, 1050.0, 200)], 1)
    verts = (centre[:, None, :] + rs.uniform(-1.0, 1.0, (200, 3, 3)) * np.array([120.0, 120.0, 60.0])).reshape(-1, 3)
    faces = np.arange(600).reshape(200, 3)
    planted_v = np.array([[np.nan, 0.0, 600.0],                                            # 600: a NaN vertex
                          [0.0, 0.0, -600.0],                                              # 601: behind the camera
                          [-50.0, -50.0, 5000.0], [50.0, -50.0, 5000.0], [0.0, 50.0, 5000.0],      # 602-604: wholly beyond far
                          [-50.0, -50.0, 900.0], [50.0, -50.0, 900.0], [0.0, 50.0, 1200.0],        # 605-607: straddles far
                          [2.0e7, 0.0, 600.0],                                             # 608: u = 2e6, beyond the guard band
                          [-200.0, 0.0, 600.0], [200.0, 0.5, 600.0], [200.0, 1.2, 600.0],          # 609-611: a sliver 0.07 pixel thin
                          [-200.0, 31.0, 600.0], [200.0, 30.0, 600.0], [200.0, 31.5, 600.0],       # 612-614: another, across pixel rows
                          [-2000.0, -2000.0, 800.0], [4000.0, -2000.0, 800.0], [-2000.0, 4000.0, 800.0],      # 615-617: the whole image
                          [-100.0, -50.0, 600.0], [100.0, -50.0, 600.0], [0.0, 100.0, 600.0],      # 618-620: on pixel centres (16,13) (36,13) (26,28)
                          [100.0, 100.0, 600.0],                                           # 621: (36,28): shares the edge 619-620
                          [-60.0, -40.0, 250.0], [40.0, -40.0, 250.0], [-10.0, 50.0, 250.0]])      # 622-624: in front of everything
    planted_f = np.array([[0, 1, 625], [-1, 0, 1], [600, 3, 4], [601, 6, 7], [602, 603, 604], [605, 606, 607], [608, 9, 10], [12, 12, 13],
                          [609, 610, 611], [612, 614, 613], [615, 616, 617], [618, 619, 620], [619, 621, 620], [620, 619, 621],
                          [622, 623, 624], [624, 623, 622], [622, 623, 624]])              # 134-136: both windings and a coplanar duplicate
    verts = np.concatenate([verts, planted_v]).astype(np.float32)
    faces = np.concatenate([faces[:120], planted_f, faces[120:]]).astype(np.int32)
    vrgb = rs.randint(0, 256, (len(verts), 3)).astype(np.uint8)
    K, E = rig(9)
    table = MR.view_table(K, E, NEAR, FAR)
    want = {(flags, moved): restate(verts, faces, table, H0, W0, flags, TRANSFORM if moved else None, vrgb)
            for flags, moved in ((0, False), (_lib.RASTER_CULL_NEG, False), (_lib.RASTER_CULL_POS, False), (0, True))}
    for w in want.values():
        for a in w:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    c = want[(0, False)][1]
    assert (c[1, [0, 1, 2, 3, 4, 6]] > 0).all() and c[1, 0] == 3 and (c[:, 5] == 0).all() and c[:, 7].min() > 50      # every slot is met (5: below)
    assert want[(_lib.RASTER_CULL_NEG, False)][1][1, 5] > 50 and want[(_lib.RASTER_CULL_POS, False)][1][1, 5] > 50
    f = want[(0, False)][4]
    assert (f[1] >= 0).all() and (f == 130).any()                                          # the whole-image face fills view 1
    assert (f[1] == 134).any() and not np.isin(f, (135, 136)).any()                        # equal depths go to the smaller face index
    return verts, faces, vrgb, table, want


@pytest.mark.parametrize("cull,moved", [(None, False), ("neg", False), ("pos", False), (None, True)])
def test_every_output_equals_the_restatement_bitwise(ops, exact_case, cull, moved):
    verts, faces, vrgb, table, want = exact_case
    flags = {None: 0, "neg": _lib.RASTER_CULL_NEG, "pos": _lib.RASTER_CULL_POS}[cull]
    w_zid, w_counts, w_covered, w_depth, w_face, w_normal, w_rgb = want[(flags, moved)]
    zid, counts, work, depth, face, normal, rgb = run(ops, verts, faces, table, H0, W0, cull=cull, T=TRANSFORM if moved else None, vrgb=vrgb)
    assert np.array_equal(counts.cpu().numpy(), w_counts)
    assert np.array_equal(u64(zid), w_zid)
    assert int(work[0]) == w_covered and int(work[2]) == 0 and 0 < int(work[1]) <= w_covered
    assert np.array_equal(bits(depth), bits(w_depth)) and np.array_equal(face.cpu().numpy(), w_face)
    assert np.array_equal(bits(normal), bits(w_normal))
    assert np.array_equal(rgb.cpu().numpy(), w_rgb)


# ------------------------------------------------------------------------------------------ 2. watertight
KW = np.array([[4.0, 0.0, 3.0], [0.0, 4.0, 2.0], [0.0, 0.0, 1.0]])


def lattice_mesh(n, seed):
    """an n x n lattice of vertices at multiples of 0.5 on the plane z = 2 -- under KW and the identity they project onto the pixel centres
    (3 + i, 2 + j) -- with a random diagonal and a random winding per triangle"""
    rs = np.random.RandomState(seed)
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    verts = np.stack([0.5 * i.ravel(), 0.5 * j.ravel(), np.full(n * n, 2.0)], 1).astype(np.float32)
    faces = []
    for y in range(n - 1):
        for x in range(n - 1):
            a, b, c, d = y * n + x, y * n + x + 1, (y + 1) * n + x + 1, (y + 1) * n + x
            for tri in (((a, b, c), (a, c, d)) if rs.rand() < 0.5 else ((a, b, d), (b, c, d))):
                faces.append(tri if rs.rand() < 0.5 else tri[::-1])
    return verts, np.array(faces, np.int32)


@pytest.mark.parametrize("seed", [0, 1])
def test_a_lattice_on_pixel_centres_is_watertight_and_hit_once(ops, seed):
    verts, faces = lattice_mesh(12, seed)
    table = MR.view_table(KW[None], np.eye(4)[None], 0.5, 10.0)
    zid, counts, work, depth, face, _, _ = run(ops, verts, faces, table, 18, 20)
    assert counts.cpu().tolist() == [[0, 0, 0, 0, 0, 0, 0, 2 * 11 * 11]]
    mask = (face[0] >= 0).cpu().numpy()
    rows, cols = np.nonzero(mask)
    # 12 x 12 centres, of which one boundary row and one boundary column belong to no face (half-open); every other one exactly once
    assert int(work[0]) == int(mask.sum()) == 11 * 11
    assert rows.max() - rows.min() == 10 and cols.max() - cols.min() == 10 and rows.min() in (2, 3) and cols.min() in (3, 4)
    assert np.array_equal(bits(depth[0])[mask], np.full(121, np.float32(2.0).view(np.uint32)))


# ------------------------------------------------------------------------------------------ 3. every path, same bits
def straddling_mesh():
    """right triangles on pixel centres (KW, z = 2 and deeper) whose clipped boxes hold 63, 64 and 65 pixels -- just below, at and just
    above DMVS_RASTER_SMALL -- two faces over the whole 40 x 40 image and forty random small ones"""
    assert _lib.RASTER_SMALL == 64
    rs = np.random.RandomState(2)
    verts, faces = [], []

    def tri(u0, v0, w, h, z):
        px = np.array([[u0, v0], [u0 + w - 1, v0], [u0, v0 + h - 1]], np.float64)
        faces.append([len(verts), len(verts) + 1, len(verts) + 2])
        verts.extend([[(p[0] - 3.0) * z / 4.0, (p[1] - 2.0) * z / 4.0, z] for p in px])
    for n, (w, h) in enumerate([(7, 9), (9, 7), (8, 8), (8, 8), (5, 13), (13, 5), (33, 2), (3, 22)]):
        tri(2 + 3 * n, 1 + 2 * n, w, h, 2.0 + 0.25 * n)
    tri(-5, -5, 100, 100, 4.0)
    tri(60, 60, -90, -90, 3.5)
    for _ in range(40):
        tri(rs.randint(0, 36), rs.randint(0, 36), rs.randint(1, 6), rs.randint(1, 6), 1.0 + rs.randint(0, 16) / 4.0)
    return np.array(verts, np.float32), np.array(faces, np.int32)


def test_queue_and_grid_do_not_change_a_bit(ops):
    verts, faces = straddling_mesh()
    E = np.stack([np.eye(4), np.eye(4)])
    E[1, 0, 3] = 0.25
    table = MR.view_table(np.stack([KW, KW]), E, 0.5, 10.0)
    ref = run(ops, verts, faces, table, 40, 40, queue_cap=None, blocks=0)
    large = 0
    for v in range(2):
        for f in faces:
            slot, ft = setup(verts, f, table[v], 0, 40, 40)
            large += ft is not None and (ft["box"][1] - ft["box"][0] + 1) * (ft["box"][3] - ft["box"][2] + 1) > _lib.RASTER_SMALL
    assert large >= 6 and int(ref[2][2]) == 0 and int(ref[1][:, 7].sum()) > 60
    for queue_cap in (0, 1, None):
        for blocks in (1, 3, 0):
            got = run(ops, verts, faces, table, 40, 40, queue_cap=queue_cap, blocks=blocks)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (queue_cap, blocks)
            assert int(got[2][0]) == int(ref[2][0])
            # one view chunk, one queue: everything beyond its capacity falls back
            assert int(got[2][2]) == (0 if queue_cap is None else large - queue_cap), (queue_cap, blocks)
            assert all(torch.equal(a, b) for a, b in zip(got[3:6], ref[3:6]))


# ------------------------------------------------------------------------------------------ 4. analytic plane
def test_inverse_depth_of_a_plane_is_affine_within_the_snapping_bound(ops):
    """the plane z = 4 + x / 4 + y / 2 as a jittered grid whose vertices are multiples of 1 / 64 (exactly on it in fp32), seen by a
    rotated camera.  1 / depth of a plane is a u + b v + c; snapping moves a vertex by at most 1 / 512 pixel per axis, which changes an
    affine interpolant by at most (|a| + |b|) / 512 inside the triangle, and the fp32 depth adds a relative 2^-24."""
    rs = np.random.RandomState(4)
    n = 20
    gy, gx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x = np.round((gx.ravel() * 0.5 - 5.0 + rs.uniform(-0.15, 0.15, n * n)) * 64.0) / 64.0
    y = np.round((gy.ravel() * 0.5 - 5.0 + rs.uniform(-0.15, 0.15, n * n)) * 64.0) / 64.0
    verts = np.stack([x, y, 4.0 + 0.25 * x + 0.5 * y], 1)
    assert np.array_equal(verts.astype(np.float32).astype(np.float64), verts)
    faces = np.array([t for r in range(n - 1) for c in range(n - 1) for t in ((r * n + c, r * n + c + 1, (r + 1) * n + c + 1),
                                                                            (r * n + c, (r + 1) * n + c + 1, (r + 1) * n + c))], np.int32)
    H, W = 31, 37
    K = np.array([[40.0, 0.0, 18.0], [0.0, 40.0, 15.0], [0.0, 0.0, 1.0]])
    ay, ax = 0.2, -0.1
    R = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]]) @ np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, [0.3, -0.2, 0.5]
    res = MR.render_mesh(ops, verts.astype(np.float32), faces, K[None], E[None], (H, W), depth_range=(0.5, 50.0))
    # n . X = rho in the world  ->  1 / depth = (R n) . K^-1 (u, v, 1) / (rho + (R n) . t)
    nw, rho = np.array([-0.25, -0.5, 1.0]), 4.0
    coef = np.linalg.inv(K).T @ (R @ nw) / (rho + (R @ nw) @ E[:3, 3])
    depth, mask = res["depth"][0].cpu().numpy().astype(np.float64), res["mask"][0].cpu().numpy()
    rows, cols = np.nonzero(mask)
    assert mask.mean() > 0.5 and int(res["counts"][0, 1]) == 0
    want = coef[0] * cols + coef[1] * rows + coef[2]
    err = np.abs(1.0 / depth[mask] - want).max()
    bound = (abs(coef[0]) + abs(coef[1])) / 512.0 + 2.0 ** -22 * want.max()
    print(f"plane: max |1/depth - affine| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------------------------------ 5. closing the loop
def look_at(c):
    z = -c / np.linalg.norm(c)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, np.cross(z, x), z])
    E[:3, 3] = -E[:3, :3] @ c
    return E


def test_a_fused_sphere_renders_back_to_its_depth_maps(ops):
    """analytic depth maps of the unit sphere -> tsdf_integrate -> tsdf_extract -> render_mesh into the same views.  A surface-nets vertex
    lies inside its cell, so the surface is within sqrt(3) h of the sphere; along a ray of incidence cosine >= 0.5 that is at most
    2 sqrt(3) h of depth."""
    H = W = 48
    n, V = 40, 6
    h = 2.5 / (n - 1)
    K = np.array([[1.1 * W, 0.0, W / 2.0], [0.0, 1.1 * W, H / 2.0], [0.0, 0.0, 1.0]])
    Es = np.stack([look_at(3.4 * d) for d in np.concatenate([np.eye(3), -np.eye(3)])])
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T
    depth, cosine = np.zeros((V, H, W)), np.zeros((V, H, W))
    for v in range(V):
        c = Es[v, :3, 3]                                       # the sphere's centre in the camera frame
        a, b, cc = (ray * ray).sum(-1), -2.0 * (ray @ c), c @ c - 1.0
        disc = b * b - 4 * a * cc
        t = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
        hit = disc > 0
        depth[v] = np.where(hit, t, 0.0)
        normal = t[..., None] * ray - c
        cosine[v] = np.where(hit, -(normal * ray).sum(-1) / np.sqrt(a), 0.0)
    d32 = dev(ops, depth.astype(np.float32))
    vol = ops.tsdf_volume((n, n, n), [-1.25, -1.25, -1.25], h, colour=False)
    ops.tsdf_integrate(vol, d32, d32 > 0, None, M.tsdf_views(np.repeat(K[None], V, 0), Es), 4 * h)
    verts, _, faces = ops.tsdf_extract(vol, min_weight=1)
    assert faces.shape[0] > 1000
    res = MR.render_mesh(ops, verts, faces, np.repeat(K[None], V, 0), Es, (H, W), depth_range=(0.5, 10.0))
    got, drawn = res["depth"].cpu().numpy().astype(np.float64), res["mask"].cpu().numpy()
    silhouette = depth > 0
    judged = silhouette & (cosine >= 0.5) & drawn
    err = np.abs(got - depth)[judged].max()
    print(f"sphere: {judged.sum()} of {silhouette.sum()} silhouette pixels judged, max error {err:.4f}, bound {2 * np.sqrt(3) * h:.4f}")
    assert judged.sum() >= 0.6 * silhouette.sum()
    assert err <= 2.0 * np.sqrt(3.0) * h
    assert int(res["counts"][:, :2].sum()) == 0 and int(res["counts"][:, 7].min()) > 500


# ------------------------------------------------------------------------------------------ 6. tree round trip
def plane_mesh(spacing=25.0):
    """the plane of synth_scene(seed = 3) as a grid mesh with random vertex colours"""
    d0, a, c = synth.scene_plane(3)
    xs, ys = np.arange(-450.0, 451.0, spacing), np.arange(-350.0, 351.0, spacing)
    gx, gy = np.meshgrid(xs, ys, indexing="xy")
    verts = np.stack([gx.ravel(), gy.ravel(), d0 + a * gx.ravel() + c * gy.ravel()], 1).astype(np.float32)
    w = len(xs)
    faces = np.array([t for r in range(len(ys) - 1) for q in range(w - 1) for t in ((r * w + q, r * w + q + 1, (r + 1) * w + q + 1),
                                                                                   (r * w + q, (r + 1) * w + q + 1, (r + 1) * w + q))], np.int32)
    rgb = np.random.RandomState(6).randint(40, 256, (len(verts), 3)).astype(np.uint8)
    return verts, rgb, faces


def test_command_line_round_trip(ops, tmp_path, capsys):
    from PIL import Image
    from diffmvs_amd import depth_eval as DE, train_driver as TD
    sc = synth.synth_scene(48, 64, n_views=5, n_src=2, seed=3, grid_w=3)
    tree, prev = str(tmp_path / "tree"), str(tmp_path / "preview")
    write_tree(tree, sc)
    verts, rgb, faces = plane_mesh()
    IO.write_ply(str(tmp_path / "mesh.ply"), verts, rgb, faces=faces)
    res = MR.main(["--mesh", str(tmp_path / "mesh.ply"), "--tree", tree, "--preview", prev], ops=ops)
    assert list(res["scans"]) == [""] and len(res["scans"][""]["views"]) == 5 and res["faces"] == len(faces)
    record = json.load(open(os.path.join(tree, "render.json")))
    assert record["not_drawn_near_plane"] == 0 and record["views"]["00000000"]["size"] == [32, 64]
    assert all(sum(r[k] for k in MR.SLOT_NAMES) == len(faces) and r["not_drawn_near_plane"] == 0 and r["covered"] > 0.9 for r in record["views"].values())
    # what the tree's readers see is what render_mesh returns for load_view's cameras
    ds = IO.MVSDataset(tree, dataset="general")
    views = [ds.load_view("", v) for v in range(5)]
    direct = MR.render_mesh(ops, verts, faces, np.stack([v[1] for v in views]), np.stack([v[2] for v in views]), (32, 64),
                            depth_range=[(v[3], v[4]) for v in views])
    train = TD.TreeTrainSet(tree, [""], 3, numdepth=8, dataset="general")
    s = train.get(0, None)
    ref = s["view_ids"][0]
    assert len(train) == 5 and torch.equal(s["depth"]["stage4"], direct["depth"][ref].cpu()) and torch.equal(s["mask"]["stage4"] > 0.5, direct["mask"][ref].cpu())
    for v in range(5):
        mask = np.array(Image.open(os.path.join(tree, "mask", f"{v:08d}.png"))) > 0
        assert np.array_equal(mask, direct["mask"][v].cpu().numpy())
        shaded = np.array(Image.open(os.path.join(prev, f"{v:08d}.png")))
        assert shaded.shape == (32, 64, 3) and np.array_equal(shaded.any(-1), mask)      # non-black exactly where the mask is set
    # depth_eval of an estimate that IS the ground truth: zero error over exactly the masked pixels
    os.makedirs(tmp_path / "est" / "depth_est")
    for v in range(5):
        IO.save_pfm(str(tmp_path / "est" / "depth_est" / f"{v:08d}.pfm"), IO.read_pfm(os.path.join(tree, "depth_gt", f"{v:08d}.pfm"))[0])
    capsys.readouterr()
    score = DE.main(["--outdir", str(tmp_path / "est"), "--gtpath", tree], ops=ops)
    assert score["overall"]["abs_err"] == 0.0 and score["counters"]["views"] == 5
    assert score["counters"]["masked"] == score["counters"]["scored"] == int(direct["mask"].sum()) > 0
    # a second run refuses before anything is written
    before = files(str(tmp_path))
    with pytest.raises(SystemExit, match="--overwrite"):
        MR.main(["--mesh", str(tmp_path / "mesh.ply"), "--tree", tree, "--cull", "neg", "--preview", str(tmp_path / "preview2")], ops=ops)
    assert files(str(tmp_path)) == before and not os.path.exists(tmp_path / "preview2")
    # the plane faces one way: culling one sign keeps every face of a view, culling the other none
    MR.main(["--mesh", str(tmp_path / "mesh.ply"), "--tree", tree, "--cull", "pos", "--overwrite"], ops=ops)
    again = json.load(open(os.path.join(tree, "render.json")))["views"]
    assert all(again[k]["culled"] in (0, record["views"][k]["drawn"] + record["views"][k]["off_image"]) for k in again)


# ------------------------------------------------------------------------------------------ 7. argument checks (CPU only)
def test_rejected_arguments_return_einval_before_any_launch():
    """the pointers (other than the host tables, which the checks read) are never dereferenced"""
    from diffmvs_amd.build import build_hip
    dll = _lib.Lib(build_hip()).dll
    p, odd, odd8 = C.c_void_p(4096), C.c_void_p(4098), C.c_void_p(4100)      # odd8: 4-byte but not 8-byte aligned
    good = MR.view_table(K0[None].repeat(2, 0), np.stack([np.eye(4)] * 2), 1.0, 100.0)

    def zid(table=good, **kw):
        a = dict(verts=p, N=10, faces=p, F=5, transform=None, V=len(table), H=8, W=8, flags=0, blocks=0, zid=p, counts=p, work=p, queue=p, queue_cap=4)
        a.update(kw)
        t = np.ascontiguousarray(table, np.float64)
        tr = None if a["transform"] is None else (C.c_double * 12)(*a["transform"])
        return dll.dmvs_mesh_raster_zid_u64(a["verts"], a["N"], a["faces"], a["F"], tr, t.ctypes.data_as(C.c_void_p) if a["V"] else None, a["V"], a["H"],
                                            a["W"], a["flags"], a["blocks"], a["zid"], a["counts"], a["work"], a["queue"], a["queue_cap"], None)

    def resolve(table=good, **kw):
        a = dict(zid=p, verts=p, N=10, faces=p, F=5, transform=None, V=len(table), H=8, W=8, vrgb=p, depth=p, face=p, normal=p, rgb=p)
        a.update(kw)
        t = np.ascontiguousarray(table, np.float64)
        tr = None if a["transform"] is None else (C.c_double * 12)(*a["transform"])
        return dll.dmvs_mesh_raster_resolve_f32(a["zid"], a["verts"], a["N"], a["faces"], a["F"], tr, t.ctypes.data_as(C.c_void_p), a["V"], a["H"], a["W"],
                                                a["vrgb"], a["depth"], a["face"], a["normal"], a["rgb"], None)

    def table(col, value):
        t = good.copy()
        t[1, col] = value
        return t
    for fn in (zid, resolve):
        for kw in (dict(N=-1), dict(F=-1), dict(V=-1), dict(H=-1), dict(W=-1)):                      # a negative size
            assert fn(**kw) == -22, (fn.__name__, kw)
        assert fn(N=2 ** 31) == -22 and fn(F=2 ** 31) == -22 and fn(H=2 ** 16, W=2 ** 15) == -22      # N, F, H W >= 2^31
        assert fn(table=np.repeat(good, 600, 0), H=2 ** 15, W=2 ** 15) == -22                        # V H W > 2^40
        assert fn(faces=None) == -22 and fn(verts=None) == -22 and fn(zid=None) == -22               # NULL operands with work to do
        assert fn(verts=odd) == -22 and fn(faces=odd) == -22 and fn(zid=odd8) == -22                 # 4 and 8 byte alignment
        for col in (0, 7, 8, 19):
            assert fn(table=table(col, np.nan)) == -22 and fn(table=table(col, np.inf)) == -22       # a non-finite view entry
        assert fn(table=table(20, 0.0)) == -22 and fn(table=table(20, -1.0)) == -22 and fn(table=table(20, np.nan)) == -22      # near <= 0
        assert fn(table=table(21, 1.0)) == -22 and fn(table=table(21, 0.5)) == -22                   # far <= near
        assert fn(table=table(21, 1e39)) == -22 and fn(table=table(21, np.inf)) == -22               # far > FLT_MAX
        assert fn(transform=[1.0] * 11 + [np.nan]) == -22 and fn(transform=[np.inf] + [0.0] * 11) == -22
    assert zid(counts=None) == -22 and zid(counts=odd8) == -22 and zid(work=odd8) == -22 and zid(queue=odd8) == -22
    assert zid(flags=_lib.RASTER_CULL_NEG | _lib.RASTER_CULL_POS) == -22 and zid(flags=4) == -22 and zid(flags=-1) == -22
    assert zid(blocks=-1) == -22 and zid(queue_cap=-1) == -22 and zid(queue=None, queue_cap=1) == -22
    assert resolve(depth=None) == -22 and resolve(face=None) == -22 and resolve(vrgb=None) == -22
    assert resolve(depth=odd) == -22 and resolve(face=odd) == -22 and resolve(normal=odd) == -22
    fill = dll.dmvs_mesh_raster_fill_u64
    assert fill(p, -1, None) == -22 and fill(None, 8, None) == -22 and fill(odd8, 8, None) == -22 and fill(p, 2 ** 40 + 1, None) == -22
    assert fill(None, 0, None) == 0                                                                  # nothing to do: nothing touched
