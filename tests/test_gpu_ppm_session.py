"""GPU: resumable photon mapping (cgrt_ppm_session).  After photons added in any chunks totalling k, the session's image,
rgb8 and hitpoints must equal cgrt_ppm_render with nphotons = k bit for bit -- and through it the compiled reference's
golden vectors and the oracle -- whatever the chunks, batch, pair buffer halvings, lookahead or producer overlap."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from backends import BackendScene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
import make_golden  # noqa: E402

CHUNKS = [1, 2999, 7000]  # then the rest; with batch=3000 the chunks straddle batch boundaries


def _canon(hp, spp):
    ps = hp[:, 0].astype(np.int64)
    pix, smp = ps // spp, ps % spp
    out = np.concatenate([pix[:, None].astype(np.float64), smp[:, None].astype(np.float64), hp[:, 2:]], axis=1)
    order = np.lexsort([out[:, 7], out[:, 6], out[:, 5], out[:, 1], out[:, 0]])
    return out[order]


def _feed(ses, total, chunks=CHUNKS):
    for c in chunks:
        ses.add_photons(c)
    ses.add_photons(total - sum(chunks))
    assert ses.photons_done == total


def _case(name):
    return {c[0]: c for c in make_golden.photon_cases() + make_golden.photon_cases_bezier()}[name]


@pytest.mark.parametrize("case", make_golden.photon_cases(), ids=[c[0] for c in make_golden.photon_cases()])
def test_chunked_session_matches_reference_golden(gpu_ready, case):
    import cgraytracing_amd as cg
    name, mk, cam, W, H, spp, nph = case
    g = np.load(os.path.join(GOLD, "ppm_%s.npz" % name))
    with cg.Scene(mk()) as sc:
        one = sc.ppm_render(W, H, spp, cam(), 5, 12345, nphotons=nph)
        with sc.ppm_session(W, H, spp, cam(), 5, 12345, batch=3000) as ses:
            _feed(ses, nph)
            img, hp, inf = ses.image(), ses.hitpoints(), ses.info()
    got = _canon(hp, spp)
    assert got.shape == g["hp"].shape
    assert np.array_equal(got, g["hp"]), "hitpoints (geometry, flux, r2, n)"
    assert np.array_equal(img, g["image"]), "gathered image"
    assert inf["photons_done"] == nph and inf["hp_count"] == len(hp) == one["count"]
    assert inf["n_events"] == one["n_events"]
    assert inf["device_bytes"] > 0 and inf["ms_photons"] > 0


@pytest.mark.parametrize("name", ["c2_48x36", "bump_40x30"])
def test_checkpoints_match_one_shot_and_oracle(gpu_ready, orc, name):
    import cgraytracing_amd as cg
    _, mk, cam, W, H, spp, nph = _case(name)
    objs = mk()
    o = BackendScene(orc, objs)
    with cg.Scene(objs) as sc, sc.ppm_session(W, H, spp, cam(), 5, 12345) as ses:
        for k in (1000, 5000, 12345, nph):
            ses.add_photons(k - ses.photons_done)
            img, rgb8 = ses.image(), ses.rgb8()
            one = sc.ppm_render(W, H, spp, cam(), 5, 12345, nphotons=k, want_rgb8=True)
            want = o.ppm(cam(), W, H, spp, 5, nphotons=k)["image"]
            assert np.array_equal(img, one["image"]), k
            assert np.array_equal(img, want), k
            assert np.array_equal(rgb8, one["rgb8"]) and np.array_equal(rgb8, orc.tonemap(img)), k
            assert ses.info()["n_events"] == one["n_events"], k


def test_batch_machinery_across_calls(gpu_ready, monkeypatch):
    """pair_cap forced low, so batches are halved (and grow back) inside calls and the reduced batch size carries over call
    boundaries; lookahead on and off; a call of fewer photons than a batch right after a lookahead (the batch traced ahead
    is dropped); and everything on the null stream (CGRT_PHOTON_OVERLAP=0).  All must equal the golden image."""
    import cgraytracing_amd as cg
    name, mk, cam, W, H, spp, nph = _case("c2_48x36")
    g = np.load(os.path.join(GOLD, "ppm_%s.npz" % name))
    chunks = [1, 2999, 500, 7000, 37]  # 500: fewer photons than the lookahead [3000, 5999) traced for it, which is dropped
    with cg.Scene(mk()) as sc:
        base = sc.ppm_render(W, H, spp, cam(), 5, 12345, nphotons=nph)
        cap = max(64, base["n_pairs"] // 40)  # room for a few hundred photons' pairs: a 3000-photon batch halves repeatedly
        runs = []
        for lookahead, overlap in ((True, None), (False, None), (True, "0")):
            if overlap is not None:
                monkeypatch.setenv("CGRT_PHOTON_OVERLAP", overlap)
            for pair_cap in (0, cap):
                with sc.ppm_session(W, H, spp, cam(), 5, 12345, batch=3000, pair_cap=pair_cap, lookahead=lookahead) as ses:
                    halvings = []
                    for c in chunks + [nph - sum(chunks)]:
                        before = ses.info()["n_batch_halvings"]
                        ses.add_photons(c)
                        halvings.append(ses.info()["n_batch_halvings"] - before)
                    runs.append((lookahead, overlap, pair_cap, halvings, ses.image(), ses.hitpoints(), ses.info()))
            monkeypatch.delenv("CGRT_PHOTON_OVERLAP", raising=False)
    for lookahead, overlap, pair_cap, halvings, img, hp, inf in runs:
        tag = (lookahead, overlap, pair_cap, halvings)
        assert np.array_equal(img, g["image"]), tag
        assert np.array_equal(hp, runs[0][5]), tag
        assert inf["n_events"] == base["n_events"], tag
        if pair_cap:
            # the 2999-photon call overflows and halves; its reduced batch is where the calls after it start, and later calls
            # (the batch grown back as radii shrink) overflow again
            assert sum(halvings) >= 3 and halvings[1] >= 1 and sum(1 for h in halvings if h) >= 2, tag
        else:
            assert sum(halvings) == 0, tag


def test_sessions_by_rows_assemble_to_full_frame(gpu_ready):
    """Ranks that own a band or block-cyclic stripes each hold a session fed the same chunks; at every checkpoint their rows
    equal the full-frame session's (and the assembled stripes the whole frame)."""
    import torch
    import cgraytracing_amd as cg
    from cgraytracing_amd import dist as cdist
    objs = scenes.planes(scenes.stone_small_texture(True)) + [scenes.Sphere((5, -12, 30), 5, (1, 1, 1), 0.8, 0.5)]
    W, H, spp, n, S = 56, 40, 2, 3, 8
    rows_local = cdist.local_rows(H, S, 0, n)
    kw = dict(camera=scenes.cam_dof(), max_depth=5, seed=12345, batch=3000)
    with cg.Scene(objs) as sc:
        full = sc.ppm_session(W, H, spp, **kw)
        band = sc.ppm_session(W, H, spp, rows=16, row_offset=8, **kw)
        ranks = [sc.ppm_session(W, H, spp, rows=rows_local, stripe=(S, r, n), **kw) for r in range(n)]
        for chunk in ([1, 2999, 7000], [20000]):
            for ses in [full, band] + ranks:
                for c in chunk:
                    ses.add_photons(c)
            ref = full.image()
            assert np.array_equal(band.image(), ref[8:24])
            frame = cdist.assemble(torch.from_numpy(np.stack([r.image() for r in ranks])), H, S, n).numpy()
            assert np.array_equal(frame, ref)
        last = sc.ppm_render(W, H, spp, nphotons=30000, **kw)["image"]
    assert np.array_equal(ref, last) and ref.max() > 0.5


def test_device_image_on_a_side_stream(gpu_ready):
    import torch
    import cgraytracing_amd as cg
    _, mk, cam, W, H, spp, nph = _case("c2_48x36")
    with cg.Scene(mk()) as sc, sc.ppm_session(W, H, spp, cam(), 5, 12345, nphotons=7000) as ses:
        dev = torch.device("cuda", sc.device)
        side = torch.cuda.Stream(dev)
        for k in (7000, nph):
            ses.add_photons(k - ses.photons_done)
            with torch.cuda.stream(side):
                rgb = torch.full((H, W, 3), 7, dtype=torch.uint8, device=dev)
                img = ses.image_tensor(rgb8_out=rgb)
            img2 = ses.image_tensor(stream=side.cuda_stream)
            side.synchronize()
            want = ses.image()
            assert np.array_equal(img.cpu().numpy(), want) and np.array_equal(img2.cpu().numpy(), want)
            assert np.array_equal(rgb.cpu().numpy(), ses.rgb8())
        assert ses.info()["ms_last_image"] >= 0


def test_device_image_then_photons_at_once(gpu_ready):
    """A gather on a caller's stream is still reading the Hitpoints when add_photons comes: the photons wait for it.  The image
    is the host image of that photon count bit for bit, the photons after it leave what a session without an image has, and
    the device image's time is there without a host image in between.  32 x 24, spp 2, four batches a call."""
    import torch
    import cgraytracing_amd as cg
    w, h, spp2, n = 32, 24, 2, 3000
    with cg.Scene(scenes.scene_c2()) as sc:
        dev = torch.device("cuda", sc.device)
        side = torch.cuda.Stream(dev)
        kw = dict(camera=scenes.cam_dof(), max_depth=5, seed=12345, nphotons=n, batch=800)
        with sc.ppm_session(w, h, spp2, **kw) as plain, sc.ppm_session(w, h, spp2, **kw) as ses:
            want, want_rgb = ses.image(), ses.rgb8()
            rgb = torch.full((h, w, 3), 7, dtype=torch.uint8, device=dev)
            img = ses.image_tensor(rgb8_out=rgb, stream=side.cuda_stream)
            ses.add_photons(n)
            assert ses.info()["ms_last_image"] >= 0
            side.synchronize()
            plain.add_photons(n)
            assert want.max() > 0 and np.array_equal(img.cpu().numpy(), want) and np.array_equal(rgb.cpu().numpy(), want_rgb)
            assert ses.photons_done == 2 * n and not np.array_equal(ses.image(), want)
            assert np.array_equal(ses.hitpoints(), plain.hitpoints()) and np.array_equal(ses.image(), plain.image())
            # the same with a host image between the device image and the photons
            want = ses.image()
            img = ses.image_tensor(stream=side.cuda_stream)
            host = ses.image()
            ses.add_photons(n)
            side.synchronize()
            plain.add_photons(n)
            assert np.array_equal(host, want) and np.array_equal(img.cpu().numpy(), want)
            assert ses.photons_done == 3 * n and not np.array_equal(ses.image(), want)
            assert np.array_equal(ses.hitpoints(), plain.hitpoints()) and np.array_equal(ses.image(), plain.image())


def test_session_edge_cases(gpu_ready):
    import cgraytracing_amd as cg
    from cgraytracing_amd._capi import CgrtError
    # a mirror sphere and nothing else: no eye ray ends on a diffuse surface, so the grid has no hitpoints
    with cg.Scene([scenes.Sphere((0, 0, 30), 5, (1, 1, 1), 0.8, 0.0)]) as sc, sc.ppm_session(24, 16) as ses:
        assert ses.info()["hp_count"] == 0
        ses.add_photons(5000)
        assert ses.photons_done == 5000 and ses.info()["n_events"] == 0
        assert not ses.image().any() and len(ses.hitpoints()) == 0
    name, mk, cam, W, H, spp, nph = _case("c2_48x36")
    with cg.Scene(mk()) as sc:
        with sc.ppm_session(W, H, spp, cam(), 5, 12345) as ses:
            with pytest.raises(CgrtError) as e:
                ses.image()  # before any photon: flux / (PI r2 0)
            assert e.value.code == -1
            with pytest.raises(CgrtError) as e:
                ses.add_photons(-1)
            assert e.value.code == -1
            assert ses.photons_done == 0
        with sc.ppm_session(W, H, spp, cam(), 5, 12345, rows=16, stripe=(8, 0, 2), nphotons=100) as ses:
            assert ses.image().shape == (16, W, 3)
            with pytest.raises(CgrtError) as e:
                ses.rgb8()
            assert e.value.code == -4
        # a batch is applied whole or not at all: with room for one pair, a photon's pairs overflow the buffer at some point
        with sc.ppm_session(W, H, spp, cam(), 5, 12345, pair_cap=1) as ses:
            with pytest.raises(CgrtError) as e:
                ses.add_photons(nph)
            assert e.value.code == -5
            d = ses.photons_done
            assert 0 <= d < nph
            if d:
                assert np.array_equal(ses.image(), sc.ppm_render(W, H, spp, cam(), 5, 12345, nphotons=d)["image"])
            assert len(ses.hitpoints()) == ses.info()["hp_count"]
    # two sessions of one scene, calls interleaved: each is its own one-shot render
    g1 = np.load(os.path.join(GOLD, "ppm_c2_48x36.npz"))
    _, _, cam2, W2, H2, spp2, nph2 = _case("c2_dof_32x24")
    g2 = np.load(os.path.join(GOLD, "ppm_c2_dof_32x24.npz"))
    with cg.Scene(mk()) as sc:
        a = sc.ppm_session(W, H, spp, cam(), 5, 12345, nphotons=3000)
        b = sc.ppm_session(W2, H2, spp2, cam2(), 5, 12345, batch=4000)
        b.add_photons(9000)
        a.add_photons(nph - 3000)
        assert np.array_equal(b.image(), sc.ppm_render(W2, H2, spp2, cam2(), 5, 12345, nphotons=9000)["image"])
        b.add_photons(nph2 - 9000)
        assert np.array_equal(a.image(), g1["image"]) and np.array_equal(b.image(), g2["image"])
        b.close()
    assert a._h is None  # closing the scene closed its remaining session


def test_bezier_session_equals_one_shot(gpu_ready):
    """Photons that meet the Bezier vase take Newton starts from their own keyed stream: same device code, same streams, so the
    chunked session equals the one-shot render bit for bit (both are pinned to the reference only statistically)."""
    import cgraytracing_amd as cg
    name, mk, cam, W, H, spp, nph = make_golden.photon_cases_bezier()[0]
    with cg.Scene(mk()) as sc:
        with sc.ppm_session(W, H, spp, cam(), 5, 12345, batch=1500) as ses:
            for k, c in ((1000, 1000), (nph, nph - 1000)):
                ses.add_photons(c)
                one = sc.ppm_render(W, H, spp, cam(), 5, 12345, nphotons=k, want_hitpoints=True)
                assert np.array_equal(ses.image(), one["image"]), k
                assert np.array_equal(ses.hitpoints(), one["hp"]), k
                assert ses.info()["n_events"] == one["n_events"], k


def test_cpp_progressive_example(gpu_ready, orc, tmp_path):
    """examples/ppm_progressive.cpp: C2 at 48x36, 20 000 photons in 4 passes.  The last PNG is the tone-mapped golden image of
    the compiled reference; pass 2 (10 000 photons) is the tone-mapped one-shot render of 10 000 photons."""
    from PIL import Image
    import cgraytracing_amd as cg
    exe = os.path.join(ROOT, "cgraytracing_amd", "cgrt_ppm_progressive")
    assert os.path.exists(exe), "build it with make -C cgraytracing_amd/csrc all"
    prefix = str(tmp_path / "p")
    out = subprocess.run([exe, "--scene", "c2", "--width", "48", "--height", "36", "--photons", "20000", "--passes", "4",
                          "--png-prefix", prefix], capture_output=True, text=True, timeout=300, check=True).stdout
    g = np.load(os.path.join(GOLD, "ppm_c2_48x36.npz"))
    assert "hitpoints: %d" % len(g["hp"]) in out
    png = lambda k: np.asarray(Image.open("%s%d.png" % (prefix, k)).convert("RGB"))
    assert np.array_equal(png(4), orc.tonemap(g["image"]))
    with cg.Scene(scenes.scene_c2()) as sc:
        half = sc.ppm_render(48, 36, 1, scenes.cam_pinhole(), 5, 12345, nphotons=10000, want_rgb8=True)
    assert np.array_equal(png(2), half["rgb8"])
