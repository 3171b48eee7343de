"""-m gpu: the image kernels of hope_amd/csrc/hope_bev.hip on the programmed lots of tests/image_program.py -- polygons with four
intersections, border-pass edges, one-row polygons, triangles, every span width of the QUAD fill, band / block seams, two obstacle
chunks in a band, truncation boundaries, Bresenham ties, the rotate90 switch one float32 ulp either side, crops that leave the
surface and the source, the trajectory torus at its seams and at its size limit, steps without a sub-step, a shown vehicle under
the trail.  Every comparison is uint8 equality with the oracle (which tests/test_image_program.py pins on the same lots against a
literal renderer); quarter-turn lots are also compared with the literal image directly.  Every family runs on both launches of
k_bev_image (HOPE_BEV_LEGACY forces the per-tile raster)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import image_program as P                                        # noqa: E402
from test_gpu_image import assert_images_equal, make_img_pair, restart_done      # noqa: E402

_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = P.polygons(pad=128) if name == 'polygons_padded' else getattr(P, name)()
    return _cache[name]


def assert_literal_quarter_images(img, scenes, poses, trajs, what):
    """device image == literal image (not only == oracle) wherever the heading is a quarter turn"""
    n = 0
    for k, (s, p) in enumerate(zip(scenes, poses)):
        if P.quarter_turns(p[2]) is None:
            continue
        want = P.literal_quarter_image(P.literal_world(s, p, trajs[k]), s.bbox, p)
        assert (img[k].transpose(1, 2, 0) == want).all(), f'{what}: lot {k} differs from the literal image'
        n += 1
    return n


def step_both(env, orc, act, what):
    env.step(torch.from_numpy(np.ascontiguousarray(act)).to(env.device))
    o = orc.step(act)
    torch.cuda.synchronize()
    assert np.array_equal(env.pose.cpu().numpy(), orc.pose), f'{what}: the poses differ (not an image finding)'
    return o


def run_static(fam, max_obst, steps=2):
    n = len(fam)
    assert n <= 256 and max_obst <= 160 and steps <= 4
    env, orc = make_img_pair(fam.scenes, max_obst=max_obst)
    if fam.detached:                                             # the observer is not the start pose: replaced from outside, both sides
        env.upload_state(pose=np.ascontiguousarray(fam.poses))
        orc.pose[:] = fam.poses
    env.reset_obs(); orc.reset_obs()
    img = assert_images_equal(env, orc, 'reset')
    lit = assert_literal_quarter_images(img, fam.scenes, fam.poses, [[s.start] for s in fam.scenes], 'reset')
    for it in range(steps):
        step_both(env, orc, np.tile([0.3, 0.3 if it % 2 == 0 else -0.2], (n, 1)), f'step {it}')
        assert_images_equal(env, orc, f'step {it}')
    env.close()
    return lit


def run_drive(drive, max_obst=32, literal_every=10):
    scenes = drive.family.scenes
    n = len(scenes)
    assert n <= 256 and (len(drive.actions) <= 40 or (len(drive.actions) <= 200 and n <= 16))
    env, orc = make_img_pair(scenes, max_obst=max_obst)
    env.reset_obs(); orc.reset_obs()
    assert_images_equal(env, orc, 'reset')
    for it, act in enumerate(drive.actions):
        step_both(env, orc, act, f'step {it}')
        img = assert_images_equal(env, orc, f'step {it}')
        if it % literal_every == literal_every - 1:
            assert_literal_quarter_images(img, scenes, orc.pose, orc.traj, f'step {it}')
    return env, orc


STATIC = {'polygons': 128, 'truncation': 32, 'outlines': 32, 'headings': 32}


@pytest.mark.parametrize('legacy', [False, True], ids=['layer', 'per_tile_raster'])
@pytest.mark.parametrize('name', list(STATIC))
def test_static_family(name, legacy, monkeypatch):
    if legacy:
        monkeypatch.setenv('HOPE_BEV_LEGACY', '1')
    fam = family(name)
    lit = run_static(fam, STATIC[name])
    assert lit >= (len(fam) if name != 'headings' else len(fam.facts['quarter']))


def test_polygons_beyond_the_register_resident_obstacle_chunks():
    """max_obst = 160 and every programmed obstacle at an index >= 128: the per-tile re-conversion path"""
    fam = family('polygons_padded')
    assert all(len(s.verts) > 128 for s in fam.scenes)
    run_static(fam, 160)


@pytest.mark.parametrize('legacy', [False, True], ids=['layer', 'per_tile_raster'])
def test_trails(legacy, monkeypatch):
    if legacy:
        monkeypatch.setenv('HOPE_BEV_LEGACY', '1')
    env, orc = run_drive(P.trails())
    env.close()


@pytest.mark.parametrize('legacy', [False, True], ids=['layer', 'per_tile_raster'])
def test_long_trails_across_the_layer_refresh(legacy, monkeypatch):
    if legacy:
        monkeypatch.setenv('HOPE_BEV_LEGACY', '1')
    env, orc = run_drive(P.trails(long=True), literal_every=48)
    assert min(len(t) for t in orc.traj) == 21                   # (the oracle keeps 21 of the > 193 entries)
    env.close()


@pytest.mark.parametrize('legacy', [False, True], ids=['layer', 'per_tile_raster'])
def test_shown_vehicle(legacy, monkeypatch):
    if legacy:
        monkeypatch.setenv('HOPE_BEV_LEGACY', '1')
    d = P.shown_vehicle()
    env, orc = run_drive(d)
    new = np.ascontiguousarray(orc.pose + d.replace)
    env.upload_state(pose=new)
    orc.pose[:] = new
    env.reset_obs(); orc.reset_obs()                             # the action-less step: observes again, the trajectory stays
    assert all(len(t) == 21 for t in orc.traj)                # (25 entries, of which the oracle keeps 21)
    img = assert_images_equal(env, orc, 'shown vehicle')
    assert assert_literal_quarter_images(img, d.family.scenes, new, orc.traj, 'shown vehicle') >= 100
    env.close()


def test_trails_with_auto_reset_against_restart_by_hand():
    """a torus that is cleared by an episode turnover inside the step: second handle, restart by hand, as in
    test_image_with_auto_reset_and_active_mask"""
    d = P.trails()
    scenes = d.family.scenes
    envA, orc = make_img_pair(scenes, max_obst=32)
    envB, _ = make_img_pair(scenes, max_obst=32)
    envA.reset_obs(); envB.reset_obs(); orc.reset_obs()
    n_done = 0
    for it, act in enumerate(d.actions):
        a = torch.from_numpy(np.ascontiguousarray(act)).to(envA.device)
        envA.step(a, auto_reset=True)
        envB.step(a)
        orc.step(act)
        torch.cuda.synchronize()
        n_done += int(envB.done.sum())
        restart_done(envB, orc)
        torch.cuda.synchronize()
        assert torch.equal(envA.img, envB.img), it
        assert_images_equal(envA, orc, f'auto-reset step {it}')
    assert n_done >= 4, n_done
    envA.close(); envB.close()
