"""GPU: stochastic progressive photon mapping (cgrt_sppm_session).  One pass at alpha = 1 is anchored to the pinned photon pass
(PpmSession on the same grid / rays); several passes are checked bit for bit against a replay in Python floats that uses none
of the code under test: the CPU oracle's Hitpoints and photon events, the candidate enumeration that
test_gpu_ppm_rays.lookat_expected writes out (27 cells -> buckets, duplicates kept) and steps 3-5 of include/cgrt.h.

Shape: C2 under the thin lens, 40 x 12 pixels (40 is no multiple of the 32-pixel tile), spp 2, initial_radius 2.0, 2000 photons
a pass, batch 3000 unless stated.  At the default radius 200/768 only a few per cent of the pixels are reached by 2000
photons, which is why the radius is raised; the replay's own numbers are asserted to say that the cases are not vacuous."""
import math

import numpy as np
import pytest

import scenes
from backends import BackendScene
from test_gpu_ppm_rays import EPS, PI_REF, _ref_coord, _ref_hash

pytestmark = pytest.mark.gpu

W, H, SPP, R0, NPH, SEED = 40, 12, 2, 2.0, 2000, 12345
KW = dict(initial_radius=R0, batch=3000)


class Replay:
    """The semantics of include/cgrt.h in Python floats.  hitpoints(k) -> (hp [n,9] = f, pos, normal; texel [n]) of pass k in
    emission order (texel-major, then sample, then the ray tree's order); events(first, count) -> [m,10] = photon, P, n, flux
    in serial order."""

    def __init__(self, npix, spp, hitpoints, events, r0=R0, alpha=0.7, hashsize=1000001):
        self.npix, self.spp, self.alpha, self.hashsize = npix, spp, alpha, hashsize
        self.hitpoints, self.events = hitpoints, events
        self.r02 = r0 * r0
        self.cl = 70.0 / math.ceil(70.0 / r0)  # hash.h:25-26
        self.N = [0.0] * npix
        self.R2 = [self.r02] * npix
        self.tau = [[0.0, 0.0, 0.0] for _ in range(npix)]
        self.done = self.passes = 0
        self.Mp = [0.0] * npix
        self.cnt = [0.0] * npix
        self.dup_pairs = self.n_pairs = 0
        self.history = []  # (pixels, image or None) after every pass

    def run_pass(self, M):
        hp, texel = self.hitpoints(self.passes)
        n = len(hp)
        bucket = np.array([_ref_hash(*_ref_coord(hp[i, 3:6], self.cl), self.hashsize) for i in range(n)], np.int64)
        order = np.argsort(bucket, kind="stable")  # the table: (bucket, emission order)
        hp, texel, bucket = hp[order], texel[order], bucket[order]
        f, pos, nrm = hp[:, 0:3], hp[:, 3:6], hp[:, 6:9]
        members = {}
        for i, b in enumerate(bucket):
            members.setdefault(int(b), []).append(i)
        members = {b: np.array(v, np.int64) for b, v in members.items()}
        r2 = np.array([self.R2[t] for t in texel], np.float64)  # step 1: every Hitpoint searches with its texel's radius
        phi = [[0.0, 0.0, 0.0] for _ in range(n)]
        m = [0.0] * n
        inv_pi = 1.0 / PI_REF
        for ev in (self.events(self.done, M) if M and n else ()):
            Pe, ne, fe = ev[1:4], [float(v) for v in ev[4:7]], [float(v) for v in ev[7:10]]
            ix, iy, iz = _ref_coord(Pe, self.cl)
            cand = [members[b] for b in (_ref_hash(ix - 1 + dx, iy - 1 + dy, iz - 1 + dz, self.hashsize)
                                         for dx in range(3) for dy in range(3) for dz in range(3)) if b in members]
            if not cand:
                continue
            c = np.concatenate(cand)  # a bucket is walked once per cell that hashes to it
            dd = pos[c] - Pe
            d2 = dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2]
            dn = nrm[c, 0] * ne[0] + nrm[c, 1] * ne[1] + nrm[c, 2] * ne[2]
            acc = c[(dn > EPS) & (d2 <= r2[c])]
            self.dup_pairs += len(acc) - len(set(acc.tolist()))
            self.n_pairs += len(acc)
            for h in acc.tolist():  # step 3
                phi[h] = [phi[h][k] + (float(f[h, k]) * fe[k]) * inv_pi for k in range(3)]
                m[h] += 1.0
        per_texel = [[] for _ in range(self.npix)]
        for i, t in enumerate(texel):
            per_texel[int(t)].append(i)
        for p, idx in enumerate(per_texel):
            Phi, Mp = [0.0, 0.0, 0.0], 0.0
            for i in idx:  # step 4, in table order
                Phi = [Phi[k] + phi[i][k] for k in range(3)]
                Mp += m[i]
            if Mp > 0:  # step 5
                Nn = self.N[p] + self.alpha * Mp
                g = Nn / (self.N[p] + Mp)
                self.R2[p] = self.R2[p] * g
                self.tau[p] = [(self.tau[p][k] + Phi[k]) * g for k in range(3)]
                self.N[p] = Nn
            self.Mp[p], self.cnt[p] = Mp, float(len(idx))
        self.done += M
        self.passes += 1
        self.history.append((self.pixels(), self.image() if self.done else None))
        return self

    def pixels(self):
        return np.array([[self.N[p], self.R2[p]] + self.tau[p] + [self.Mp[p], self.cnt[p], 0.0] for p in range(self.npix)], np.float64)

    def image(self):
        out = np.zeros((self.npix, 3))
        for p in range(self.npix):
            sc = 1.0 / (PI_REF * self.R2[p] * (float(self.done) * self.spp))
            out[p] = [self.tau[p][k] * sc for k in range(3)]
        return out


def oracle_replay(orc, objs, cam, w, h, spp, npasses, nph=NPH, **kw):
    o = BackendScene(orc, objs)

    def hitpoints(k):
        r = o.trace_grid(cam, w, h, spp, 5, SEED, sample0=k * spp, capture=True)
        return r["hp"], r["hp_pix"]  # the capture is serial: emission order

    rp = Replay(w * h, spp, hitpoints, lambda first, count: o.photon_events(first, count, depth=5), **kw)
    for _ in range(npasses):
        rp.run_pass(nph)
    o.close()
    return rp


_C2 = {}


def c2_replay(orc):
    """four passes of the shape above, computed once"""
    if "rp" not in _C2:
        _C2["rp"] = oracle_replay(orc, scenes.scene_c2(), scenes.cam_dof(), W, H, SPP, 4)
    return _C2["rp"]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _fold_flux(hp, texel, npix):
    tau, cnt = np.zeros((npix, 3)), np.zeros(npix)
    for i in range(len(hp)):  # table order: the per-pixel index order inside every texel
        tau[texel[i]] = tau[texel[i]] + hp[i, 11:14]
        cnt[texel[i]] += hp[i, 15]
    return tau, cnt


def _check_anchor(ses, want_hp, want_inf, texel):
    hp, px, inf = ses.last_hitpoints(), ses.pixels(), ses.info()
    assert len(hp) > 2 * W * H and _same(hp, want_hp), "all 16 columns of the table"
    assert inf["n_events"] == want_inf["n_events"] > 0 and inf["n_pairs"] == want_inf["n_pairs"] > 0
    assert inf["hp_count"] == len(hp) and inf["passes"] == 1 and inf["photons_done"] == NPH
    tau, cnt = _fold_flux(want_hp, texel, W * H)
    assert (cnt > 0).sum() >= W * H // 2
    assert np.array_equal(px[:, 0], cnt) and np.array_equal(px[:, 5], cnt)
    assert np.array_equal(px[:, 1], np.full(W * H, R0 * R0))
    assert _same(px[:, 2:5].copy(), tau)
    assert np.array_equal(px[:, 6], np.bincount(texel, minlength=W * H)) and not px[:, 7].any()


def test_one_pass_is_the_pinned_photon_pass(gpu_ready):
    import cgraytracing_amd as cg
    cam = scenes.cam_dof()
    with cg.Scene(scenes.scene_c2()) as sc:
        with sc.ppm_session(W, H, SPP, cam, 5, SEED, nphotons=NPH, alpha=1.0, **KW) as ref:
            want_hp, want_inf = ref.hitpoints(), ref.info()
        with sc.sppm_session(W, H, SPP, cam, alpha=1.0, **KW) as ses:
            ses.add_passes(1, NPH)
            _check_anchor(ses, want_hp, want_inf, want_hp[:, 0].astype(np.int64) // SPP)
        org, dirs, keys = sc.camera_rays(W, H, SPP, cam, SEED)
        with sc.ppm_session_rays(org, dirs, keys, width=W, rows=H, spp=SPP, nphotons=NPH, alpha=1.0, **KW) as ref:
            want_hp, want_inf = ref.hitpoints(), ref.info()
        with sc.sppm_session(W, H, SPP, cam, alpha=1.0, **KW) as ses:
            ses.add_pass_rays(org, dirs, NPH, keys=keys)
            _check_anchor(ses, want_hp, want_inf, want_hp[:, 0].astype(np.int64) % (W * H))


def _check_against(ses, rp, k):
    px, img = rp.history[k]
    got = ses.pixels()
    for c, name in enumerate(("N", "R2", "tau.r", "tau.g", "tau.b", "M_p", "Hitpoints", "pad")):
        assert _same(got[:, c].copy(), px[:, c].copy()), "pass %d: %s" % (k + 1, name)
    assert _same(ses.image().reshape(-1, 3), img), "pass %d: image" % (k + 1)


def test_four_passes_against_oracle_replay(gpu_ready, orc):
    import cgraytracing_amd as cg
    rp = c2_replay(orc)
    # the replay alone says that the case is not vacuous
    npix = W * H
    for k in (0, 1):
        assert (rp.history[k][0][:, 5] > 0).sum() >= npix // 2, "pass %d reaches fewer than half of the pixels" % (k + 1)
    assert (rp.history[3][0][:, 1] < R0 * R0).sum() >= npix // 2
    assert rp.history[0][0][:, 6].min() >= 2, "every pixel carries at least two Hitpoints"
    with cg.Scene(scenes.scene_c2()) as sc, sc.sppm_session(W, H, SPP, scenes.cam_dof(), **KW) as ses:
        for k in range(4):
            ses.add_passes(1, NPH)
            _check_against(ses, rp, k)
        inf = ses.info()
        assert inf["passes"] == 4 and inf["photons_done"] == 4 * NPH and inf["n_pairs"] == rp.n_pairs
        print("sppm c2: %d pairs, %d events, last pass %d Hitpoints" % (inf["n_pairs"], inf["n_events"], inf["hp_count"]))


def test_schedule_independence(gpu_ready, orc):
    import cgraytracing_amd as cg
    rp = c2_replay(orc)
    runs = []
    with cg.Scene(scenes.scene_c2()) as sc:
        for kw in (dict(batch=700), dict(batch=0), dict(batch=3000, pair_cap=2000)):
            with sc.sppm_session(W, H, SPP, scenes.cam_dof(), initial_radius=R0, **kw) as ses:
                ses.add_passes(4, NPH)
                runs.append((ses.pixels(), ses.image(), ses.rgb8(), ses.info()["n_batch_halvings"]))
    assert runs[0][3] == 0 and runs[1][3] == 0 and runs[2][3] > 0, "the low pair_cap drives the halving path"
    for r in runs[1:]:
        assert _same(r[0], runs[0][0]) and _same(r[1], runs[0][1]) and np.array_equal(r[2], runs[0][2])
    assert _same(runs[0][0], rp.history[3][0])
    assert runs[0][2].shape == (H, W, 3) and runs[0][2].max() > 0


def test_bucket_collisions(gpu_ready, orc):
    import cgraytracing_amd as cg
    rp = oracle_replay(orc, scenes.scene_c2(), scenes.cam_dof(), W, H, SPP, 2, hashsize=101)
    assert rp.dup_pairs >= 1, "no photon reached a Hitpoint through two colliding cells"
    with cg.Scene(scenes.scene_c2()) as sc, sc.sppm_session(W, H, SPP, scenes.cam_dof(), hashsize=101, **KW) as ses:
        for k in range(2):
            ses.add_passes(1, NPH)
            _check_against(ses, rp, k)
        assert ses.info()["n_pairs"] == rp.n_pairs
    print("hashsize 101: %d of %d pairs are duplicates" % (rp.dup_pairs, rp.n_pairs))


def test_grid_pass_is_ray_pass(gpu_ready, orc):
    import cgraytracing_amd as cg
    rp = c2_replay(orc)
    cam = scenes.cam_dof()
    with cg.Scene(scenes.scene_c2()) as sc, sc.sppm_session(W, H, SPP, cam, **KW) as grid, sc.sppm_session(W, H, SPP, cam, **KW) as rays:
        for k in range(3):
            grid.add_passes(1, NPH)
            org, dirs, keys = sc.camera_rays(W, H, SPP, cam, SEED, sample_offset=k * SPP)
            rays.add_pass_rays(org, dirs, NPH, keys=keys, pixel=None)
            assert _same(rays.pixels(), grid.pixels()), k
            assert _same(rays.pixels(), rp.history[k][0]), k
        assert _same(rays.image(), grid.image()) and np.array_equal(rays.rgb8(), grid.rgb8())


def test_stripes_reproduce_the_full_frame(gpu_ready):
    import cgraytracing_amd as cg
    from cgraytracing_amd import dist as cdist
    from cgraytracing_amd._capi import CgrtError
    Hf, S, n = 24, 8, 2
    cam = scenes.cam_dof()
    rows_local = cdist.local_rows(Hf, S, 0, n)
    with cg.Scene(scenes.scene_c2()) as sc:
        full = sc.sppm_session(W, Hf, SPP, cam, **KW)
        shares = [sc.sppm_session(W, Hf, SPP, cam, rows=rows_local, stripe=(S, r, n), **KW) for r in range(n)]
        for ses in [full] + shares:
            ses.add_passes(3, NPH)
        fpx, fimg = full.pixels().reshape(Hf, W, 8), full.image()
        assert (fpx[:, :, 1] < R0 * R0).sum() >= W * Hf // 2
        seen = 0
        for r, ses in enumerate(shares):
            px, img = ses.pixels().reshape(rows_local, W, 8), ses.image()
            for j in range(rows_local):
                g = cdist.global_row(j, S, r, n)
                if g < Hf:
                    assert _same(px[j].copy(), fpx[g].copy()) and _same(img[j].copy(), fimg[g].copy()), (r, j, g)
                    seen += 1
            with pytest.raises(CgrtError) as e:
                ses.rgb8()
            assert e.value.code == -4
        assert seen == Hf
        # the first pass fixed the stripes
        with pytest.raises(CgrtError) as e:
            shares[0]._grid["stripe"] = (S, 1, n)
            shares[0].add_passes(1, NPH)
        assert e.value.code == -1 and shares[0].passes == 3
        assert full.rgb8().shape == (Hf, W, 3)


def test_empty_cases(gpu_ready):
    import cgraytracing_amd as cg
    import torch
    from cgraytracing_amd._capi import CgrtError
    npix = W * H
    with cg.Scene(scenes.scene_c2()) as sc, sc.sppm_session(W, H, SPP, scenes.cam_dof(), **KW) as ses:
        dev = torch.device("cuda", sc.device)
        with pytest.raises(CgrtError) as e:
            ses.image()  # before any photon
        assert e.value.code == -1
        ses.add_passes(1, 0)  # captures, counts the pass, changes nothing else
        inf, px = ses.info(), ses.pixels()
        assert inf["passes"] == 1 and inf["photons_done"] == 0 and inf["hp_count"] > 2 * npix and inf["n_events"] == 0
        assert not px[:, 0].any() and np.array_equal(px[:, 1], np.full(npix, R0 * R0)) and not px[:, 2:6].any()
        assert px[:, 6].sum() == inf["hp_count"]
        with pytest.raises(CgrtError) as e:
            ses.image()
        assert e.value.code == -1
        ses.add_passes(1, NPH)
        before = ses.pixels()
        assert (before[:, 0] > 0).sum() >= npix // 2
        # rays that produce no Hitpoint (dir = 0 is not traced): only the counters move
        zero = torch.zeros((npix * SPP, 3), dtype=torch.float64, device=dev)
        ses.add_pass_rays(zero, zero, 500)
        inf, px = ses.info(), ses.pixels()
        assert inf["passes"] == 3 and inf["photons_done"] == NPH + 500 and inf["hp_count"] == 0 and len(ses.last_hitpoints()) == 0
        assert _same(px[:, :5].copy(), before[:, :5].copy()) and not px[:, 5:].any()
        # rays without a texel, and no rays at all
        org, dirs, keys = sc.camera_rays(W, H, SPP, scenes.cam_dof(), SEED)
        ses.add_pass_rays(org, dirs, 0, keys=keys, pixel=torch.full((npix * SPP,), -1, dtype=torch.int64, device=dev))
        ses.add_pass_rays(zero[:0], zero[:0], 0)
        ses.add_passes(1, 0)
        inf, px = ses.info(), ses.pixels()
        assert inf["passes"] == 6 and inf["photons_done"] == NPH + 500
        assert _same(px[:, :5].copy(), before[:, :5].copy())
        img = ses.image().reshape(-1, 3)
        want = before[:, 2:5] * (1.0 / (PI_REF * before[:, 1] * (float(NPH + 500) * SPP)))[:, None]
        assert _same(img, want)
        with pytest.raises(CgrtError) as e:
            ses.add_passes(1, -1)
        assert e.value.code == -1 and ses.passes == 6


def test_bounded_memory_and_monotonic_state(gpu_ready):
    import cgraytracing_amd as cg
    with cg.Scene(scenes.scene_c2()) as sc, sc.sppm_session(W, H, SPP, scenes.cam_dof(), **KW) as ses:
        px, byts = [], []
        for k in range(8):
            ses.add_passes(1, NPH)
            ses.image()
            px.append(ses.pixels())
            byts.append(ses.info()["device_bytes"])
        print("device_bytes per pass:", byts)
        assert byts[7] <= byts[1]
        for a, b in zip(px, px[1:]):
            assert (b[:, 1] <= a[:, 1]).all() and (b[:, 0] >= a[:, 0]).all()
        assert (px[7][:, 1] < px[1][:, 1]).sum() >= W * H // 2


def test_device_image_then_pass_at_once(gpu_ready):
    """An image on a caller's stream is still reading the texels when the next pass comes: the pass waits for it.  The image is
    the host image of that pass count bit for bit, and the pass after it leaves the texels and Hitpoints of a session that took
    no image.  32 x 24, four batches a pass."""
    import cgraytracing_amd as cg
    import torch
    w, h, n = 32, 24, 3000
    kw = dict(initial_radius=R0, batch=800)
    with cg.Scene(scenes.scene_c2()) as sc:
        dev = torch.device("cuda", sc.device)
        side = torch.cuda.Stream(dev)
        with sc.sppm_session(w, h, SPP, scenes.cam_dof(), **kw) as plain, sc.sppm_session(w, h, SPP, scenes.cam_dof(), **kw) as ses:
            ses.add_passes(1, n)
            want, want_rgb = ses.image(), ses.rgb8()
            rgb = torch.full((h, w, 3), 7, dtype=torch.uint8, device=dev)
            img = ses.image_tensor(rgb8_out=rgb, stream=side.cuda_stream)
            ses.add_passes(1, n)
            side.synchronize()
            plain.add_passes(2, n)
            assert want.max() > 0 and _same(img.cpu().numpy(), want) and np.array_equal(rgb.cpu().numpy(), want_rgb)
            assert ses.passes == 2 and not _same(ses.image(), want)
            assert _same(ses.pixels(), plain.pixels()) and _same(ses.last_hitpoints(), plain.last_hitpoints())
            # the same with a host image between the two, while the caller's stream is still busy with work of its own in
            # front of the device image: the pass comes behind both images
            want = ses.image()
            with torch.cuda.stream(side):
                torch.cuda._sleep(20000000)
            img = ses.image_tensor(stream=side.cuda_stream)
            host = ses.image()
            ses.add_passes(1, n)
            side.synchronize()
            plain.add_passes(1, n)
            assert _same(host, want) and _same(img.cpu().numpy(), want) and not _same(ses.image(), want)
            assert ses.passes == 3 and _same(ses.pixels(), plain.pixels()) and _same(ses.last_hitpoints(), plain.last_hitpoints())


def test_example_sppm_dof(gpu_ready, tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import sppm_dof
    out = sppm_dof.main(str(tmp_path / "dof"), 64, 36, 4, 5000, (1, 4))
    assert sorted(out) == [1, 4] and os.path.getsize(str(tmp_path / "dof_004.png")) > 0
    (a, ia), (b, ib) = out[1], out[4]
    assert a.shape == b.shape == (36, 64, 3) and a.max() > 0 and not np.array_equal(a, b)
    assert ia["passes"] == 1 and ib["passes"] == 4 and ib["photons_done"] == 20000


def test_mesh_scene_against_oracle_replay(gpu_ready, orc):
    """the golden bunny_40 shape: the glass bunny over the chessboard floor, 40 x 40, pinhole, spp 1"""
    import cgraytracing_amd as cg
    objs, cam = scenes.scene_c3(True), scenes.cam_pinhole()
    rp = oracle_replay(orc, objs, cam, 40, 40, 1, 2)
    assert (rp.history[0][0][:, 5] > 0).sum() >= 800 and (rp.history[1][0][:, 1] < R0 * R0).sum() >= 800
    with cg.Scene(objs) as sc, sc.sppm_session(40, 40, 1, cam, **KW) as ses:
        for k in range(2):
            ses.add_passes(1, NPH)
            _check_against(ses, rp, k)
        assert ses.info()["n_pairs"] == rp.n_pairs
