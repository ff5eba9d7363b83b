"""Mesh cleaning and scoring (csrc/mesh_clean.hip, diffmvs_amd/mesh_clean.py, diffmvs_amd/mesh_eval.py) against numpy restatements of the
contract in include/dmvs.h at tolerance zero: min-label iteration to its fixpoint, the area and sampling formulas in fp64 with the integer
steps in uint32 / int64.  Every kernel test runs on the host emulation here and on the MI355X under -m gpu."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
from diffmvs_amd import _lib, cloud_eval as CE, formats as IO, mesh as M, mesh_clean as MC, mesh_eval as ME


# ------------------------------------------------------------------------------------------ the contract, restated
def in_range(faces, N):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((faces >= 0) & (faces < N)).all(1)


def restate_labels(faces, N):
    """min-label iteration to a fixpoint: a face's vertices take the smallest of their labels, a vertex its label's label.  At the fixpoint
    every face's labels are equal and lab[lab] == lab: lab[v] is the smallest vertex index of v's component"""
    fv = np.asarray(faces, np.int64).reshape(-1, 3)
    fv = fv[in_range(fv, N)]
    lab = np.arange(N, dtype=np.int64)
    while True:
        new = lab.copy()
        if len(fv):
            np.minimum.at(new, fv.ravel(), np.repeat(lab[fv].min(1), 3))
        new = np.minimum(new, new[new])
        if np.array_equal(new, lab):
            return lab.astype(np.int32)
        lab = new


def sync_rounds(faces, N):
    """rounds of the SAME hook and shortcut rules when every launch reads a snapshot taken at its start (no lane sees another's writes
    inside a launch), up to and including the first round that changes nothing"""
    fv = np.asarray(faces, np.int64).reshape(-1, 3)
    fv = fv[in_range(fv, N)]
    lab, rounds = np.arange(N, dtype=np.int64), 0
    while True:
        rounds += 1
        new = lab.copy()
        m = lab[lab][fv].min(1)
        for k in range(3):
            np.minimum.at(new, lab[fv[:, k]], m)
            np.minimum.at(new, fv[:, k], m)
        new = np.minimum(new, new[new])
        if np.array_equal(new, lab):
            return rounds
        lab = new


def restate_tally(verts, faces, label, scale, cap):
    verts, faces, N = np.asarray(verts, np.float32), np.asarray(faces, np.int64).reshape(-1, 3), len(verts)
    ok = in_range(faces, N)
    P = verts[np.clip(faces, 0, max(N - 1, 0))].astype(np.float64)
    with np.errstate(all="ignore"):
        a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        cx, cy, cz = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
        fin = np.isfinite(area) & ok
        q = np.rint(np.minimum(np.where(fin, area, 0.0) * scale, cap)).astype(np.int64)
    q[~fin] = 0
    comp_faces, comp_area = np.zeros(N, np.int64), np.zeros(N, np.int64)
    r = np.asarray(label, np.int64)[faces[ok, 0]]
    np.add.at(comp_faces, r, 1)
    np.add.at(comp_area, r, q[ok])
    return q, comp_faces, comp_area


def restate_samples(verts, faces, area_cum, a0, Mn):
    verts, faces = np.asarray(verts, np.float32).astype(np.float64), np.asarray(faces, np.int64)
    k = np.arange(Mn, dtype=np.int64)
    t = k * np.int64(a0) + (np.int64(a0) >> 1)
    f = np.searchsorted(np.asarray(area_cum, np.int64), t, side="right")      # the smallest f with area_cum[f] > t
    ku = k.astype(np.uint32)
    r1 = (ku * np.uint32(3242174889)).astype(np.float64) * 2.0 ** -32
    r2 = (ku * np.uint32(2447445414)).astype(np.float64) * 2.0 ** -32
    flip = r1 + r2 > 1.0
    r1, r2 = np.where(flip, 1.0 - r1, r1), np.where(flip, 1.0 - r2, r2)
    p0, p1, p2 = (verts[faces[f, j]] for j in range(3))
    pts = (p0 + r1[:, None] * (p1 - p0)) + r2[:, None] * (p2 - p0)
    return pts.astype(np.float32), f.astype(np.int32)


# ------------------------------------------------------------------------------------------ meshes
def dev(ops, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


def uv_sphere(rings=32, segs=64):
    """the unit sphere: two poles and rings - 1 parallels of segs vertices; closed, one component"""
    th = np.pi * np.arange(1, rings) / rings
    ph = 2.0 * np.pi * np.arange(segs) / segs
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(segs))], -1).reshape(-1, 3)
    verts = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]]).astype(np.float32)
    at = lambda r, s: 1 + r * segs + s % segs      # noqa: E731
    faces = [(0, at(0, s), at(0, s + 1)) for s in range(segs)]
    for r in range(rings - 2):
        for s in range(segs):
            faces += [(at(r, s), at(r + 1, s), at(r + 1, s + 1)), (at(r, s), at(r + 1, s + 1), at(r, s + 1))]
    faces += [(len(verts) - 1, at(rings - 2, s + 1), at(rings - 2, s)) for s in range(segs)]
    return verts, np.array(faces, np.int32)


def fragment(n_faces, centre, size=0.05):
    """a fan of n_faces triangles around `centre`: one small component"""
    ang = np.linspace(0.0, 1.5 * np.pi, n_faces + 1)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.cos(3 * ang)], 1) * size
    verts = (np.concatenate([[[0.0, 0.0, 0.0]], rim]) + np.asarray(centre)).astype(np.float32)
    return verts, np.array([(0, 1 + k, 2 + k) for k in range(n_faces)], np.int32)


def join(parts):
    verts, faces, off = [], [], 0
    for v, f in parts:
        verts.append(v)
        faces.append(f + off)
        off += len(v)
    return np.concatenate(verts), np.concatenate(faces).astype(np.int32)


FRAGMENTS = [fragment(3, (3.0, 0.0, 0.0)), fragment(7, (0.0, 3.0, 0.0)), fragment(1, (0.0, 0.0, 3.0))]


def no_rounds(info):
    """the rounds to the fixpoint depend on timing on the device; nothing else in `info` does"""
    return {k: v for k, v in info.items() if k != "rounds"}


def labels(ops, faces, N, **kw):
    lab, info = MC.components(ops, dev(ops, faces), N, **kw)
    return lab.cpu().numpy(), info


def grid_tiles(n=264, tiles=4):
    """an n x n vertex grid whose quads are cut along the borders of tiles x tiles blocks: tiles^2 components"""
    idx = np.arange(n * n).reshape(n, n)
    t = n // tiles
    r, c = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    keep = ((r % t) != t - 1) & ((c % t) != t - 1)
    r, c = r[keep], c[keep]
    a, b, cc, d = idx[r, c], idx[r, c + 1], idx[r + 1, c + 1], idx[r + 1, c]
    return np.concatenate([np.stack([a, b, cc], 1), np.stack([a, cc, d], 1)]).astype(np.int32), n * n


def strip(seed, quads=4096):
    """a strip of quads under a random vertex permutation: one component whose diameter is the strip's length"""
    n = 2 * (quads + 1)
    perm = np.random.RandomState(seed).permutation(n)
    q = np.arange(quads)
    f = np.concatenate([np.stack([2 * q, 2 * q + 1, 2 * q + 3], 1), np.stack([2 * q, 2 * q + 3, 2 * q + 2], 1)])
    return perm[f].astype(np.int32), n


# ------------------------------------------------------------------------------------------ 1. labels, tolerance zero
def test_labels_of_random_faces_equal_the_restatement(ops):
    rs = np.random.RandomState(11)
    N = 3000
    faces = rs.randint(0, N - 50, (2500, 3)).astype(np.int32)      # the last 50 vertices are in no face
    faces[17], faces[900], faces[2499] = (5, -1, 9), (N, 3, 4), (1, 2, 2 ** 31 - 1)
    want = restate_labels(faces, N)
    got, info = labels(ops, faces, N)
    assert info["bad_faces"] == 3 and np.array_equal(got, want) and got.dtype == np.int32
    assert np.array_equal(got[N - 50:], np.arange(N - 50, N)) and len(np.unique(want)) > 100      # isolated vertices keep themselves
    again, info2 = labels(ops, faces, N, blocks=2, per_read=1)
    assert np.array_equal(again, got) and info2["bad_faces"] == 3


def test_labels_of_a_permuted_strip_and_the_rounds_jump_pointers(ops):
    faces, N = strip(3)
    assert N == 8194
    got, info = labels(ops, faces, N, per_read=1)
    assert np.array_equal(got, restate_labels(faces, N)) and (got == 0).all() and info["bad_faces"] == 0
    # the synchronous order of the same rules needs R_sync rounds (14 to 15 for five seeds on the CPU); a factor 2 covers the asynchronous
    # order and stale loads.  Propagation without the grandparent step needs hundreds of rounds on this input.
    r_sync = sync_rounds(faces, N)
    print(f"rounds {info['rounds']}, R_sync {r_sync}")
    assert r_sync <= 20 and info["rounds"] <= 2 * r_sync + 2
    assert np.array_equal(labels(ops, faces, N, per_read=3)[0], got)


def test_labels_of_a_tiled_grid_do_not_depend_on_blocks(ops):
    faces, N = grid_tiles()
    want = restate_labels(faces, N)
    assert len(np.unique(want)) == 16
    for blocks in (1, 3, 0):      # one workgroup, several grid passes, the library's choice
        got, info = labels(ops, faces, N, blocks=blocks)
        assert np.array_equal(got, want) and info["bad_faces"] == 0, blocks


def test_labels_of_touching_and_of_separate_tetrahedra(ops):
    tet = np.array([(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)], np.int32)
    shared = np.concatenate([tet + 3, tet])                          # vertices 3..6 and 0..3: vertex 3 is in both
    got, _ = labels(ops, shared, 7)
    assert np.array_equal(got, np.zeros(7, np.int32))
    apart = np.concatenate([tet + 4, tet])                           # the shared vertex duplicated: 4..7 and 0..3
    got, _ = labels(ops, apart, 8)
    assert np.array_equal(got, np.array([0, 0, 0, 0, 4, 4, 4, 4], np.int32))


def test_labels_of_empty_inputs(ops):
    got, info = labels(ops, np.zeros((0, 3), np.int32), 5)
    assert np.array_equal(got, np.arange(5)) and info == {"rounds": 1, "bad_faces": 0}
    got, info = labels(ops, np.array([(0, 1, 2)], np.int32), 0)      # N = 0: only the zeroed counters are touched
    assert got.shape == (0,) and info == {"rounds": 1, "bad_faces": 0}


# ------------------------------------------------------------------------------------------ 3. tallies
def tally_mesh():
    verts, faces = join([uv_sphere()] + FRAGMENTS)
    n = len(verts)
    verts = np.concatenate([verts, [[5.0, 5.0, 5.0], [5.0, 5.0, 5.0], [6.0, 5.0, 5.0], [np.nan, 0.0, 0.0], [7.0, 7.0, 7.0], [7.0, 8.0, 7.0]]]).astype(np.float32)
    extra = [(n, n + 1, n + 2), (n + 3, n + 4, n + 5), (n + 4, n + 5, len(verts))]      # zero area; a NaN vertex; out of range
    return verts, np.concatenate([faces, np.array(extra, np.int32)])


def test_tallies_equal_the_restatement_as_integers(ops):
    verts, faces = tally_mesh()
    N, F = len(verts), len(faces)
    label = restate_labels(faces, N)
    scale, cap = MC.area_scale(dev(ops, verts), F)
    assert np.frexp(scale)[0] == 0.5 and cap * F < 2.0 ** 62
    q, cf, ca = restate_tally(verts, faces, label, scale, cap)
    assert q[-3] == 0 and q[-2] == 0 and q[-1] == 0 and cf.sum() == F - 1 and (q[:-3] > 0).all()
    for blocks in (1, 0):
        got = [t.cpu().numpy() for t in ops.mesh_face_tally(dev(ops, verts), dev(ops, faces), dev(ops, label), scale, cap, blocks=blocks)]
        assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int64
        assert np.array_equal(got[0], q) and np.array_equal(got[1], cf) and np.array_equal(got[2], ca), blocks
    tab = MC.component_table(ops, verts, faces, dev(ops, label))
    roots = np.nonzero(cf)[0]
    assert np.array_equal(tab["roots"].cpu().numpy(), roots) and np.array_equal(tab["faces"].cpu().numpy(), cf[roots])
    assert np.array_equal(tab["area_fixed"].cpu().numpy(), ca[roots]) and np.array_equal(tab["area_q"].cpu().numpy(), q) and tab["scale"] == scale
    assert abs(float(tab["area"][0]) - 4.0 * np.pi) < 0.02 * 4.0 * np.pi      # (the inscribed polyhedron)


# ------------------------------------------------------------------------------------------ 4. clean
def test_clean_drops_the_fragments_and_keeps_the_order(ops):
    sv, sf = uv_sphere()
    rgb = np.random.RandomState(2).randint(0, 256, (len(sv), 3)).astype(np.uint8)
    frag_v, frag_f = join(FRAGMENTS)
    frag_rgb = np.full((len(frag_v), 3), 9, np.uint8)
    lone = np.array([[9.0, 9.0, 9.0]], np.float32)      # a vertex no face names
    # fragments behind the sphere
    verts, faces = join([(sv, sf), (frag_v, frag_f), (lone, np.zeros((0, 3), np.int32))])
    v, c, f, info = MC.clean(ops, verts, np.concatenate([rgb, frag_rgb, [[1, 2, 3]]]).astype(np.uint8), faces, min_faces=10)
    assert torch.equal(v.cpu(), torch.from_numpy(sv)) and torch.equal(c.cpu(), torch.from_numpy(rgb)) and torch.equal(f.cpu(), torch.from_numpy(sf))
    assert f.dtype == torch.int32 and info["components"] == 4 and info["kept"] == 1 and info["faces_removed"] == 11
    assert info["vertices_removed"] == len(frag_v) + 1 and info["bad_faces"] == 0 and info["largest_faces"] == len(sf)
    assert abs(info["largest_area"] - 4.0 * np.pi) < 0.02 * 4.0 * np.pi and info["rounds"] >= 2
    # fragments in front: the same faces after the offset
    verts2, faces2 = join([(lone, np.zeros((0, 3), np.int32)), (frag_v, frag_f), (sv, sf)])
    v2, c2, f2, info2 = MC.clean(ops, verts2, None, faces2, min_faces=10)
    assert c2 is None and torch.equal(v2.cpu(), torch.from_numpy(sv)) and torch.equal(f2.cpu(), torch.from_numpy(sf))
    assert torch.equal(torch.from_numpy(faces2[len(frag_f):] - (1 + len(frag_v))), f2.cpu()) and info2["vertices_removed"] == len(frag_v) + 1
    # the three rules agree here, and an out-of-range face goes with the fragments
    bad = np.concatenate([faces, [[0, 1, len(verts)]]]).astype(np.int32)
    a = MC.clean(ops, verts, None, bad, keep_largest=1)
    b = MC.clean(ops, verts, None, bad, min_fraction=0.5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[2].cpu(), torch.from_numpy(sf)) and no_rounds(a[3]) == no_rounds(b[3])
    assert a[3]["bad_faces"] == 1 and a[3]["faces_removed"] == 12
    # keep_largest counts by faces: the sphere, then the 7-fan
    two = MC.clean(ops, verts, None, faces, keep_largest=2)
    assert two[3]["kept"] == 2 and int(two[2].shape[0]) == len(sf) + 7
    # a clean mesh comes back as it was
    v3, c3, f3, info3 = MC.clean(ops, sv, rgb, sf, min_faces=10)
    assert torch.equal(v3.cpu(), torch.from_numpy(sv)) and torch.equal(c3.cpu(), torch.from_numpy(rgb)) and torch.equal(f3.cpu(), torch.from_numpy(sf))
    assert info3["faces_removed"] == 0 and info3["vertices_removed"] == 0 and info3["components"] == 1
    v4, _, f4, info4 = MC.clean(ops, verts, None, faces)      # no rule: only the unnamed vertex goes
    assert info4["kept"] == 4 and info4["faces_removed"] == 0 and info4["vertices_removed"] == 1 and torch.equal(f4.cpu(), torch.from_numpy(faces))


# ------------------------------------------------------------------------------------------ 5. samples, bit for bit
def check_samples(ops, verts, faces, spacing):
    pts, face_of, s = ME._sample(ops, verts, faces, spacing)
    area_q = s["area_q"].cpu().numpy()
    scale, cap = MC.area_scale(dev(ops, verts), len(faces))
    assert s["scale"] == scale and np.array_equal(area_q, restate_tally(verts, faces, np.zeros(len(verts), np.int64), scale, cap)[0])
    a0 = max(1, int(np.rint(spacing ** 2 * scale)))
    Mn = int(area_q.sum()) // a0
    assert s["a0"] == a0 and tuple(pts.shape) == (Mn, 3) and tuple(face_of.shape) == (Mn,)
    want_p, want_f = restate_samples(verts, faces, np.cumsum(area_q), a0, Mn)
    got_p, got_f = pts.cpu().numpy(), face_of.cpu().numpy()
    assert got_p.dtype == np.float32 and got_f.dtype == np.int32
    assert np.array_equal(got_f, want_f) and np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
    counts = np.bincount(got_f, minlength=len(faces))
    assert (np.abs(counts - area_q / a0) <= 1.0).all() and (counts[area_q == 0] == 0).all()      # systematic sampling: within one of the share
    both = ME.sample_surface(ops, verts, faces, spacing)
    assert torch.equal(both[0], pts) and torch.equal(both[1], face_of)
    return got_p, Mn


def test_samples_equal_the_restatement_bitwise(ops):
    verts, faces = tally_mesh()
    faces = faces[:-1]
    pts, Mn = check_samples(ops, verts, faces, 0.05)
    assert 4500 < Mn < 5500
    on = np.linalg.norm(pts.astype(np.float64), axis=1)
    assert (on[np.abs(pts).max(1) < 2.0] <= 1.0 + 1e-6).all() and (on <= 1.0 + 1e-6).sum() > 4400      # the sphere's samples lie inside it
    sv, sf = uv_sphere()
    pts, Mn = check_samples(ops, sv, sf, 0.1)
    assert 0 < Mn < len(sf) and (np.linalg.norm(pts.astype(np.float64), axis=1) <= 1.0 + 1e-6).all()
    square = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    pts, Mn = check_samples(ops, square, np.array([(0, 1, 2), (0, 2, 3)], np.int32), 1.0 / 64.0)
    assert Mn == 4096 and (pts >= 0).all() and (pts <= 1).all()
    cells = np.bincount((np.minimum(pts[:, 0] * 8, 7).astype(int) * 8 + np.minimum(pts[:, 1] * 8, 7).astype(int)), minlength=64)
    assert cells.min() > 32 and cells.max() < 96      # 64 per cell of the square if even
    with pytest.raises(_lib.DmvsError, match="would fit"):
        ME.sample_surface(ops, square, np.array([(0, 1, 2), (0, 2, 3)], np.int32), 1e-5)


# ------------------------------------------------------------------------------------------ 6. scoring
def test_scores_of_a_mesh_are_the_scores_of_its_samples(ops):
    sv, sf = uv_sphere()
    spacing, max_dist, thr = 0.08, 0.5, [0.02, 0.1]
    pts = ME.sample_surface(ops, sv, sf, spacing)[0]
    gt = (pts.cpu().numpy().astype(np.float64) * 1.01).astype(np.float32)
    res = ME.evaluate_mesh(ops, sv, sf, gt, spacing, max_dist, thr)
    want = CE.evaluate(ops, pts, gt, max_dist, thr)
    assert {k: res[k] for k in want} == want and sorted(set(res) - set(want)) == ["area", "samples", "spacing"]
    assert res["samples"] == len(pts) and res["spacing"] == spacing and abs(res["area"] - 4 * np.pi) < 0.02 * 4 * np.pi and 0 < res["accuracy"] < 0.02
    own = ME.evaluate_mesh(ops, sv, sf, pts, spacing, max_dist, thr)
    assert own["accuracy"] == 0.0 and own["completeness"] == 0.0 and own["fscore"] == [1.0, 1.0]
    fv, ff = fragment(40, (3.0, 0.0, 0.0), size=0.5)
    verts, faces = join([(sv, sf), (fv, ff)])
    dirty = ME.evaluate_mesh(ops, verts, faces, pts, spacing, max_dist, thr)
    assert dirty["samples"] > own["samples"] and dirty["precision"][1] < own["precision"][1] == 1.0
    fixed = ME.evaluate_mesh(ops, verts, faces, pts, spacing, max_dist, thr, min_faces=100)
    assert fixed["cleaned"]["kept"] == 1 and fixed["precision"] == own["precision"] and fixed["samples"] == own["samples"]
    with pytest.raises(TypeError):
        ME.evaluate_mesh(ops, sv, sf, pts, spacing, max_dist, thr, density=0.1)


# ------------------------------------------------------------------------------------------ 7. argument checks (CPU only)
def test_rejected_arguments_return_einval_before_any_launch():
    """the pointers are never dereferenced"""
    from diffmvs_amd.build import build_hip
    dll = _lib.Lib(build_hip()).dll
    p, odd, odd8 = C.c_void_p(4096), C.c_void_p(4098), C.c_void_p(4100)      # odd8: 4-byte but not 8-byte aligned

    def label(**kw):
        a = dict(faces=p, F=5, N=10, label=p, state=p, blocks=0)
        a.update(kw)
        return dll.dmvs_mesh_label_round_i32(a["faces"], a["F"], a["N"], a["label"], a["state"], a["blocks"], None)

    def tally(**kw):
        a = dict(verts=p, N=10, faces=p, F=5, label=p, scale=1024.0, cap=1e6, area_q=p, comp_faces=p, comp_area=p, blocks=0)
        a.update(kw)
        return dll.dmvs_mesh_face_tally_i64(a["verts"], a["N"], a["faces"], a["F"], a["label"], a["scale"], a["cap"], a["area_q"], a["comp_faces"],
                                            a["comp_area"], a["blocks"], None)

    def sample(**kw):
        a = dict(verts=p, N=10, faces=p, F=5, area_cum=p, a0=4, M=7, points=p, face_of=p, blocks=0)
        a.update(kw)
        return dll.dmvs_mesh_sample_f32(a["verts"], a["N"], a["faces"], a["F"], a["area_cum"], a["a0"], a["M"], a["points"], a["face_of"], a["blocks"], None)

    for fn in (label, tally, sample):
        assert fn(N=-1) == -22 and fn(F=-1) == -22 and fn(N=2 ** 31) == -22 and fn(F=2 ** 31) == -22, fn.__name__      # sizes
        assert fn(blocks=-1) == -22 and fn(faces=None) == -22 and fn(faces=odd) == -22, fn.__name__
    assert label(label=None) == -22 and label(state=None) == -22 and label(label=odd) == -22 and label(state=odd) == -22
    assert label(state=None, F=0) == -22      # the counters are always written
    for name in ("verts", "label", "area_q", "comp_faces", "comp_area"):
        assert tally(**{name: None}) == -22, name
    for name in ("verts", "label", "comp_faces"):
        assert tally(**{name: odd}) == -22, name
    assert tally(area_q=odd8) == -22 and tally(comp_area=odd8) == -22
    for scale in (0.0, -2.0, 3.0, 1000.0, np.inf, np.nan):
        assert tally(scale=scale) == -22, scale
    assert tally(cap=-1.0) == -22 and tally(cap=np.nan) == -22 and tally(cap=np.inf) == -22 and tally(cap=2.0 ** 62) == -22
    for name in ("verts", "area_cum", "points", "face_of"):
        assert sample(**{name: None}) == -22, name
    assert sample(verts=odd) == -22 and sample(points=odd) == -22 and sample(face_of=odd) == -22 and sample(area_cum=odd8) == -22
    assert sample(a0=0) == -22 and sample(a0=-3) == -22 and sample(M=-1) == -22 and sample(M=2 ** 31) == -22 and sample(M=2 ** 31 - 1, a0=2 ** 33) == -22
    assert sample(M=0, points=None, face_of=None) == 0      # nothing to do: nothing touched


# ------------------------------------------------------------------------------------------ 8. command lines
def test_command_lines_round_trip(ops, tmp_path, capsys):
    sv, sf = uv_sphere()
    fv, ff = fragment(5, (3.0, 0.0, 0.0), size=0.5)
    verts, faces = join([(fv, ff), (sv, sf)])
    rgb = np.random.RandomState(4).randint(0, 256, (len(verts), 3)).astype(np.uint8)
    src, out, gt, samples = (str(tmp_path / n) for n in ("in.ply", "out.ply", "gt.ply", "samples.ply"))
    IO.write_ply(src, verts, rgb, faces=faces)
    res = MC.main(["--mesh", src, "--out", out, "--min_faces", "10"], ops=ops)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == {"mesh_clean": res}
    v, c, f = IO.read_ply_mesh(out)
    assert np.array_equal(v, sv) and np.array_equal(c, rgb[len(fv):]) and np.array_equal(f, sf)
    assert res["faces"] == len(sf) and res["vertices"] == len(sv) and res["faces_removed"] == 5 and res["kept"] == 1 and res["ply"] == out
    MC.main(["--mesh", src, "--out", str(tmp_path / "same.ply")], ops=ops)      # no rule: the file as it was
    assert open(tmp_path / "same.ply", "rb").read() == open(src, "rb").read()
    pts = ME.sample_surface(ops, sv, sf, 0.1)[0].cpu().numpy()
    IO.write_ply(gt, pts, np.zeros((len(pts), 3), np.uint8))
    capsys.readouterr()
    score = ME.main(["--mesh", src, "--gt", gt, "--spacing", "0.1", "--max_dist", "0.5", "--thresholds", "0.05", "--min_faces", "10", "--samples_ply", samples], ops=ops)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == {"mesh_eval": score}
    assert score["accuracy"] == 0.0 and score["fscore"] == [1.0] and score["samples"] == len(pts) and score["cleaned"]["faces_removed"] == 5
    assert np.array_equal(IO.read_ply(samples)[0], pts)
    unclean = ME.main(["--mesh", src, "--gt", gt, "--spacing", "0.1", "--max_dist", "0.5", "--thresholds", "0.05"], ops=ops)
    assert unclean["precision"][0] < 1.0 and "cleaned" not in unclean


def test_mesh_min_component_writes_what_clean_makes_of_the_plain_mesh(ops, tmp_path):
    sys.path.insert(0, os.path.dirname(__file__))
    import fusion_scene
    root = fusion_scene.build_tree(str(tmp_path / "scan"), noise=0.02, outliers=0.02)
    plain, flagged = str(tmp_path / "plain.ply"), str(tmp_path / "flagged.ply")
    base = ["--outdir", root, "--testpath", root, "--dataset", "dtu", "--resolution", "24", "--trunc", "3", "--min_weight", "1"]
    a = M.main(base + ["--out", plain], ops=ops)[""]
    assert sorted(a) == ["bounds", "dims", "faces", "observed_voxels", "ply", "vertices", "views", "voxel"]      # the result line as it was
    verts, rgb, faces = IO.read_ply_mesh(plain)
    IO.write_ply(str(tmp_path / "rewritten.ply"), verts, rgb, faces=faces)                               # ... and the writer's bytes
    assert open(tmp_path / "rewritten.ply", "rb").read() == open(plain, "rb").read()
    table = MC.component_table(ops, verts, faces, MC.components(ops, dev(ops, faces), len(verts))[0])
    sizes = np.sort(table["faces"].cpu().numpy())
    assert len(sizes) >= 2, "the noisy scene is expected to leave floaters"
    n = int(sizes[-1])      # everything but the largest component(s) goes
    b = M.main(base + ["--out", flagged, "--min_component", str(n)], ops=ops)[""]
    v, c, f, info = MC.clean(ops, verts, rgb, faces, min_faces=n)
    IO.write_ply(str(tmp_path / "want.ply"), v.cpu().numpy(), c.cpu().numpy(), faces=f.cpu().numpy())
    assert open(flagged, "rb").read() == open(tmp_path / "want.ply", "rb").read()
    assert no_rounds(b["cleaned"]) == no_rounds(info) and b["cleaned"]["rounds"] >= 2 and b["faces"] == int(f.shape[0]) < a["faces"] and b["vertices"] == int(v.shape[0]) < a["vertices"]
