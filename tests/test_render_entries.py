"""One scene through all eight render entries (pt_render, pt_render_adaptive, pt_render_spectral, pt_render_adaptive_spectral and their node forms) while the
film size, the bin count and the wavelength count change under the caches the entries share on a scene: the device film, the spectral planes, the packed shards,
their staging buffers, the queues and the adaptive buffers.  The other files compare each entry with its one-device twin on fresh scenes; here every result of
the one long-lived scene is compared with the same one-device call on a fresh default-tuned scene, and the resident spectral film is followed along the way."""
import numpy as np
import pytest

from test_spectral_multi import bits, same_adaptive, same_fixed, tuned_scene, pick_rel, COUNTERS

F = np.float32
A = (40, 20)    # two tiles: one of three shards is empty
B = (77, 45)    # six tiles, remnants on the right, at the bottom and in the corner
SPP, MAX_SPP, STEP = 10, 30, 10


def with_bins(r):
    """(film, counts, stats, profile) of the adaptive entries without a spectral film, in same_adaptive's order"""
    return r[0], r[1], r[2], np.zeros(1, F), r[3]


def same_film(got, ref, what):
    """(film, profile)"""
    assert np.array_equal(bits(got[0]), bits(ref[0])), what
    assert [getattr(got[1], c) for c in COUNTERS] == [getattr(ref[1], c) for c in COUNTERS], what
    assert got[1].kernel_launches[5] == ref[1].kernel_launches[5] == 0, what


def spreads(ref, what):
    """An adaptive reference (film, counts, ..., profile) exercises the rounds: counts that differ between pixels, more than one round."""
    assert ref[1].min() < ref[1].max(), (what, np.unique(ref[1]))
    assert ref[-1].kernel_launches[5] > 1, what


@pytest.mark.gpu
def test_gpu_one_scene_through_all_eight_entries(engine, pkg):
    a = pkg.api
    builder = pkg.scene.cornell_box()
    sc = tuned_scene(engine, pkg, builder, 3)
    rng = np.random.default_rng(5)

    def fresh():
        return engine.create_scene(builder)

    def desc(size, **kw):
        return a.render_desc(size[0], size[1], SPP, 4, seed=7, **kw)
    rd_a, rd_b = desc(A), desc(B)
    rel_a, rel_b = pick_rel(engine, builder, rd_a, 0.4), pick_rel(engine, builder, rd_b, 0.4)
    resident = {}

    def spectral_step(size, bins, spectral, what):
        """after a spectral step: the resident film is this call's, and develops to what the returned array develops to"""
        assert sc.spectral_resident() == (size[0], size[1], bins), what
        M = rng.uniform(-2.0, 2.0, (3, bins)).astype(F)
        want = engine.spectral_project(spectral, M)
        assert np.any(want != 0), what
        assert np.array_equal(bits(sc.spectral_project_resident(M)), bits(want)), what
        resident.update(shape=(size[0], size[1], bins), M=M, want=want)

    def other_step(what):
        """after a step without a spectral film: the resident film is still the previous spectral step's"""
        assert sc.spectral_resident() == resident["shape"], what
        assert np.array_equal(bits(sc.spectral_project_resident(resident["M"])), bits(resident["want"])), what

    assert sc.spectral_resident() is None
    # 1
    got = sc.render_spectral(rd_b, 5)
    same_fixed(got, fresh().render_spectral(rd_b, 5), 1)
    assert np.any(got[1] != 0)
    spectral_step(B, 5, got[1], 1)
    # 2: every cache is larger than needed
    same_film(sc.render(rd_a), fresh().render(rd_a), 2)
    other_step(2)
    # 3
    ref = fresh().render_adaptive(rd_b, MAX_SPP, rel_b, step=STEP, stats=True)
    spreads(ref, 3)
    same_adaptive(with_bins(sc.render_adaptive(rd_b, MAX_SPP, rel_b, step=STEP, stats=True)), with_bins(ref), 3)
    other_step(3)
    # 4
    got = sc.render_spectral_multi(rd_a, 7, device_mask=1)
    same_fixed(got, fresh().render_spectral(rd_a, 7), 4)
    spectral_step(A, 7, got[1], 4)
    # 5: the queues widen
    hero = desc(B, hero_wavelengths=4)
    same_film(sc.render(hero), fresh().render(hero), 5)
    other_step(5)
    # 6: one wavelength again
    ref_b5 = fresh().render_adaptive_spectral(rd_b, 5, MAX_SPP, rel_b, step=STEP, stats=True)
    spreads(ref_b5, 6)
    got = sc.render_adaptive_spectral(rd_b, 5, MAX_SPP, rel_b, step=STEP, stats=True)
    same_adaptive(got, ref_b5, 6)
    spectral_step(B, 5, got[3], 6)
    # 7
    film_b = fresh().render(rd_b)
    same_film(sc.render_multi(rd_b, device_mask=1), film_b, 7)
    other_step(7)
    # 8: packed shards and staging grow
    ref = fresh().render_adaptive_spectral(rd_a, 3, MAX_SPP, rel_a, step=STEP, stats=True)
    spreads(ref, 8)
    got = sc.render_adaptive_spectral_multi(rd_a, 3, MAX_SPP, rel_a, step=STEP, stats=True, device_mask=1)
    same_adaptive(got, ref, 8)
    spectral_step(A, 3, got[3], 8)
    got = sc.render_adaptive_spectral_multi(rd_b, 5, MAX_SPP, rel_b, step=STEP, stats=True, device_mask=1)
    same_adaptive(got, ref_b5, "8 B")
    spectral_step(B, 5, got[3], "8 B")
    # 9
    ref = fresh().render_adaptive(rd_a, MAX_SPP, rel_a, step=STEP, stats=True)
    spreads(ref, 9)
    same_adaptive(with_bins(sc.render_adaptive_multi(rd_a, MAX_SPP, rel_a, step=STEP, stats=True, device_mask=1)), with_bins(ref), 9)
    other_step(9)
    # 10: the planes grow by bins, not by pixels
    got = sc.render_spectral(rd_a, 64)
    same_fixed(got, fresh().render_spectral(rd_a, 64), 10)
    spectral_step(A, 64, got[1], 10)
    # 11: step 7's film
    got = sc.render(rd_b)
    same_film(got, film_b, 11)
    other_step(11)
