"""CPU, no library: the Python layer (rust-pathtracer_amd/api.py) against a recording fake of the C boundary.

ctypes.CDLL is patched so that Library binds functions that only record their arguments.  What is pinned down per method: which entry it reaches and with
how many arguments, which output pointers are None when an output is not asked for, what the returned tuple holds, which error channel a refusal's
message comes from, and the message for an entry the library lacks.  For the render_denoised* composites: the sequence of entries per route."""
import ctypes as C

import numpy as np
import pytest

W, H, BINS, G, MASK = 3, 2, 2, 2, 0b101
IDS = [0, 1, 1]
PATH = "fake.so"
SHAPES = {"film": ((H, W, 4), np.float32), "counts": ((H, W), np.uint32), "stats": ((H, W, 2), np.float64), "group_films": ((G, H, W, 4), np.float32),
          "spectral": ((BINS, H, W), np.float32), "group_spectral": ((G, BINS, H, W), np.float32), "variance": ((H, W), np.float32)}


class FakeFn:
    def __init__(self, lib, name):
        self.lib, self.name = lib, name

    def __call__(self, *args):
        lib, name = self.lib, self.name
        lib.calls.append((name, args))
        if name.endswith("last_error") or name == "device_info":
            return name.encode()
        if name in ("scene_create", "scene_create_tuned"):
            args[-1]._obj.value = 0x1000
        elif name == "resident_info":
            info = args[1]._obj
            info.width, info.height, info.bins, info.parts = W, H, BINS, lib.parts
        elif name in ("spectral_resident", "light_groups_resident", "light_groups_denoised_resident", "light_groups_spectral_resident"):
            for a, v in zip(args[1:], (W, H, BINS if name == "spectral_resident" else G, BINS)):
                a._obj.value = v
        return lib.fail.get(name, 0)


class FakeLib:
    """Exports every pt_* name but those in `missing`; every function records its call and returns PT_OK, or the status `fail` names for it."""

    def __init__(self):
        self.calls, self.missing, self.fail, self.parts, self.fns = [], set(), {}, 0, {}

    def __getattr__(self, name):
        if not name.startswith("pt_") or name[3:] in self.missing:
            raise AttributeError(name)
        return self.fns.setdefault(name, FakeFn(self, name[3:]))

    def entries(self):
        return [n for n, _ in self.calls if not n.endswith("last_error")]


class Builder:
    def __init__(self, api):
        self.api = api

    def desc(self):
        return self.api.SceneDesc(), None


@pytest.fixture
def make(pkg, monkeypatch):
    """make(missing) -> (api, fake, Library over the fake, Scene over that)."""
    api = pkg.api

    def make(missing=()):
        fake = FakeLib()
        fake.missing = set(missing)
        monkeypatch.setattr(C, "CDLL", lambda path: fake)
        lib = api.Library(PATH, "pt_")
        scene = lib.create_scene(Builder(api))
        assert fake.entries() == ["scene_create"] and scene.handle.value == 0x1000
        fake.calls.clear()
        return api, fake, lib, scene
    return make


def address(p):
    return C.cast(p, C.c_void_p).value


def check_array(a, kind, what):
    shape, dtype = SHAPES[kind]
    assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == dtype and a.flags.c_contiguous, (what, kind)


def expect_refusals(make, call, entry, channel, also_missing=()):
    """A failing status carries the channel's message when the library exports the channel and pt_last_error's when it does not; a missing entry is refused
    with PT_ERR_UNSUPPORTED and the entry's name."""
    for missing, message in (((), channel or "last_error"), ((channel,) if channel else (), "last_error")):
        api, fake, lib, scene = make(missing)
        fake.fail[entry] = 1
        with pytest.raises(api.PtError) as e:
            call(api, lib, scene)
        assert e.value.status == 1 and str(e.value) == "pt_status 1: " + message, (entry, missing)
        assert fake.entries()[-1] == entry
    api, fake, lib, scene = make((entry,) + tuple(also_missing))
    assert getattr(lib, "_" + entry) is None
    with pytest.raises(api.PtError) as e:
        call(api, lib, scene)
    assert e.value.status == api.PT_ERR_UNSUPPORTED and str(e.value) == "pt_status 4: %s has no pt_%s entry" % (PATH, entry)
    assert entry not in fake.entries()


# ---- the fourteen render methods ------------------------------------------------------------------------------------------------------------------------
# method -> (the entry's arguments after the scene handle, in the C order; the emulation error channel; the arguments of the call)
ADAPTIVE = dict(max_samples=4, rel_error=0.125, abs_error=0.5, step=2)
GROUPS = dict(instance_group=IDS)
RENDERS = {
    "render": ("rd film prof", None, {}),
    "render_multi": ("rd mask film prof", None, {}),
    "render_spectral": ("rd sd film spectral prof", None, dict(bins=BINS)),
    "render_spectral_multi": ("rd sd mask film spectral prof", None, dict(bins=BINS)),
    "render_adaptive": ("rd ad film counts stats prof", None, ADAPTIVE),
    "render_adaptive_multi": ("rd ad mask film counts stats prof", None, ADAPTIVE),
    "render_adaptive_spectral": ("rd ad sd film counts stats spectral prof", None, dict(ADAPTIVE, bins=BINS)),
    "render_adaptive_spectral_multi": ("rd ad sd mask film counts stats spectral prof", None, dict(ADAPTIVE, bins=BINS)),
    "render_light_groups": ("rd gd film group_films prof", "light_groups_last_error", GROUPS),
    "render_light_groups_multi": ("rd gd mask film group_films prof", "light_groups_last_error", GROUPS),
    "render_adaptive_light_groups": ("rd ad gd film counts stats group_films prof", "adaptive_light_groups_last_error", dict(ADAPTIVE, **GROUPS)),
    "render_adaptive_light_groups_multi": ("rd ad gd mask film counts stats group_films prof", None, dict(ADAPTIVE, **GROUPS)),
    "render_light_groups_spectral": ("rd gd sd film group_films spectral group_spectral prof", "light_groups_spectral_last_error", dict(GROUPS, bins=BINS)),
}
RENDERS_REQUIRED = ("render",)   # (bound as required: a library without it does not load)
RENDERS_UNGUARDED = ("render_multi",)   # (optional, but the method never refused a library without it by name)


def flag_cases(layout):
    layout = layout.split()
    cases = [{}]
    for flag, kind in (("stats", "stats"), ("read_groups", "group_films"), ("read_bins", "group_spectral")):
        if kind in layout:
            cases = [dict(c, **{flag: v}) for c in cases for v in (False, True)]
    return cases


@pytest.mark.parametrize("method", sorted(RENDERS))
def test_render_method(make, method):
    layout, channel, kwargs = RENDERS[method]
    layout = layout.split()
    for flags in flag_cases(" ".join(layout)):
        api, fake, lib, scene = make()
        rd = api.render_desc(W, H, 1, 2)
        kw = dict(kwargs, **flags)
        if "mask" in layout:
            kw["device_mask"] = MASK
        got = getattr(scene, method)(rd, **kw)
        assert fake.entries() == [method], flags
        args = fake.calls[0][1]
        assert len(args) == len(getattr(lib, "_" + method).argtypes) == 1 + len(layout)
        assert args[0] is scene.handle
        absent = {"stats": not flags.get("stats", False), "group_films": not flags.get("read_groups", True),
                  "spectral": not flags.get("read_bins", True), "group_spectral": not flags.get("read_bins", True)}
        returned = [k for k in layout if k in SHAPES or k == "prof"]
        if absent["stats"] and "stats" in returned:
            returned.remove("stats")
        assert isinstance(got, tuple) and len(got) == len(returned), (flags, returned)
        out = dict(zip(returned, got))
        for kind, arg in zip(layout, args[1:]):
            what = (method, flags, kind)
            if kind == "rd":
                assert arg._obj is rd, what
            elif kind == "ad":
                ad = arg._obj
                assert isinstance(ad, api.AdaptiveDesc) and (ad.max_samples, ad.step, ad.rel_error, ad.abs_error) == (4, 2, 0.125, 0.5), what
            elif kind == "gd":
                gd = arg._obj
                assert isinstance(gd, api.LightGroupsDesc) and (gd.group_count, gd.instance_count, gd.environment_group) == (G, len(IDS), 0), what
                assert [gd.instance_group[i] for i in range(len(IDS))] == IDS, what
            elif kind == "sd":
                assert isinstance(arg._obj, api.SpectralDesc) and arg._obj.bins == BINS, what
            elif kind == "mask":
                assert getattr(arg, "value", arg) == MASK, what
            elif kind == "prof":
                assert isinstance(out["prof"], api.Profile) and arg._obj is out["prof"], what
            elif absent.get(kind, False):
                assert arg is None, what
                assert kind == "stats" or out[kind] is None, what
            else:
                check_array(out[kind], kind, what)
                assert address(arg) == out[kind].ctypes.data, what
    if method in RENDERS_REQUIRED:
        with pytest.raises(AttributeError):
            make((method,))
        return
    call = lambda api, lib, scene: getattr(scene, method)(api.render_desc(W, H, 1, 2), **kwargs)
    if method in RENDERS_UNGUARDED:
        api, fake, lib, scene = make()
        fake.fail[method] = 1
        with pytest.raises(api.PtError, match="pt_status 1: last_error$"):
            call(api, lib, scene)
        return
    expect_refusals(make, call, method, channel)


def test_group_count_defaults_to_the_largest_id_plus_one(make):
    """G = the largest id + 1, the environment's group included; `groups` overrides it."""
    api, fake, lib, scene = make()
    rd = api.render_desc(W, H, 1, 2)
    for kw, want in ((dict(environment_group=4), 5), (dict(groups=3), 3), (dict(environment_group=1, groups=7), 7)):
        for method, more in (("render_light_groups", {}), ("render_light_groups_multi", {}), ("render_light_groups_spectral", dict(bins=BINS)),
                             ("render_adaptive_light_groups", ADAPTIVE), ("render_adaptive_light_groups_multi", ADAPTIVE)):
            fake.calls.clear()
            got = getattr(scene, method)(rd, instance_group=IDS, **dict(kw, **more))
            gd = next(a._obj for a in fake.calls[0][1] if isinstance(getattr(a, "_obj", None), api.LightGroupsDesc))
            assert (gd.group_count, gd.environment_group) == (want, kw.get("environment_group", 0)), (method, kw)
            assert max(a.shape[0] for a in got if isinstance(a, np.ndarray) and a.ndim >= 4) == want, (method, kw)


# ---- the four host-array filters ------------------------------------------------------------------------------------------------------------------------
def filter_inputs(**more):
    z = lambda kind: np.zeros(*SHAPES[kind])
    base = dict(film=z("film"), counts=z("counts"), stats=z("stats"), guides=z("film"))
    extra = dict(spectral=z("spectral"), group_films=z("group_films"), albedo=z("film"), bin_albedo=z("spectral"))
    return dict(base, **{k: (extra[k] if v is True else v) for k, v in more.items()})


# case -> (method, entry, channel, inputs, the entry's arguments, what comes back besides the variance)
FILTERS = {
    "film": ("denoise_film", "denoise_film", "denoise_last_error", {}, "d film counts stats guides out variance", ["film"]),
    "film_albedo": ("denoise_film", "denoise_film_albedo", "denoise_albedo_last_error", dict(albedo=True), "d film counts stats guides albedo out variance", ["film"]),
    "spectral": ("denoise_spectral", "denoise_spectral", "denoise_spectral_last_error", dict(spectral=True),
                 "d n film counts stats guides spectral out out_planes variance", ["film", "spectral"]),
    "spectral_albedo": ("denoise_spectral_albedo", "denoise_spectral_albedo", "denoise_spectral_albedo_last_error", dict(spectral=True, albedo=True, bin_albedo=True),
                        "d n film counts stats guides albedo spectral bin_albedo out out_planes variance", ["film", "spectral"]),
    "spectral_no_albedo": ("denoise_spectral_albedo", "denoise_spectral_albedo", "denoise_spectral_albedo_last_error", dict(spectral=True),
                           "d n film counts stats guides albedo spectral bin_albedo out out_planes variance", ["film", "spectral"]),
    "light_groups": ("denoise_light_groups", "denoise_light_groups", "denoise_light_groups_last_error", dict(group_films=True, albedo=True),
                     "d n film counts stats guides albedo group_films out variance out_planes", ["film", "group_films"]),
    "light_groups_no_albedo": ("denoise_light_groups", "denoise_light_groups", "denoise_light_groups_last_error", dict(group_films=True),
                               "d n film counts stats guides albedo group_films out variance out_planes", ["film", "group_films"]),
}


@pytest.mark.parametrize("case", sorted(FILTERS))
def test_filter(make, case):
    method, entry, channel, inputs, layout, kinds = FILTERS[case]
    layout = layout.split()
    for variance in (False, True):
        api, fake, lib, scene = make()
        given = filter_inputs(**inputs)
        got = getattr(lib, method)(iterations=3, sigma_luminance=2.0, sigma_depth=0.5, normal_power_log2=5, device=2, variance=variance, **given)
        assert fake.entries() == [entry]
        args = fake.calls[0][1]
        assert len(args) == len(getattr(lib, "_" + entry).argtypes) == len(layout)
        if method == "denoise_film" and not variance:
            got = (got,)
        want = kinds + (["variance"] if variance else [])
        assert isinstance(got, tuple) and len(got) == len(want)
        for a, kind in zip(got, want):
            check_array(a, kind, (case, variance))
        for kind, arg in zip(layout, args):
            what = (case, variance, kind)
            if kind == "d":
                d = arg._obj
                assert (d.width, d.height, d.iterations, d.sigma_luminance, d.sigma_depth, d.normal_power_log2, d.device) == (W, H, 3, 2.0, 0.5, 5, 2), what
            elif kind == "n":
                assert arg == (G if "group_films" in kinds else BINS), what
            elif kind == "out":
                assert address(arg) == got[0].ctypes.data, what
            elif kind == "out_planes":
                assert address(arg) == got[1].ctypes.data, what
            elif kind == "variance":
                assert (address(arg) == got[-1].ctypes.data) if variance else (arg is None), what
            elif kind in given:
                assert address(arg) == given[kind].ctypes.data, what   # (already of the entry's type and contiguous: handed over as it is)
            else:
                assert kind in ("albedo", "bin_albedo") and arg is None, what
    expect_refusals(make, lambda api, lib, scene: getattr(lib, method)(**filter_inputs(**inputs)), entry, channel)


def test_filter_shape_refusals(make):
    api, fake, lib, scene = make()
    bad = np.zeros((H + 1, W, 4), np.float32)
    one = " of one film size"
    for method, inputs, message in (
            ("denoise_film", dict(guides=bad), "film [H,W,4], counts [H,W], stats [H,W,2] and guides [H,W,4]" + one),
            ("denoise_film", dict(albedo=bad), "albedo [H,W,4] of the film's size"),
            ("denoise_spectral", dict(spectral=np.zeros((BINS, H, W + 1), np.float32)), "film [H,W,4], counts [H,W], stats [H,W,2], guides [H,W,4] and spectral [B,H,W]" + one),
            ("denoise_spectral_albedo", dict(spectral=True, guides=bad), "film [H,W,4], counts [H,W], stats [H,W,2], guides [H,W,4] and spectral [B,H,W]" + one),
            ("denoise_spectral_albedo", dict(spectral=True, albedo=bad), "albedo [H,W,4] of the film's size"),
            ("denoise_spectral_albedo", dict(spectral=True, bin_albedo=np.zeros((BINS + 1, H, W), np.float32)), "bin_albedo [B,H,W] of the spectral film's size"),
            ("denoise_light_groups", dict(group_films=np.zeros((G, H, W, 3), np.float32)),
             "film [H,W,4], counts [H,W], stats [H,W,2], guides [H,W,4] and group_films [G,H,W,4]" + one),
            ("denoise_light_groups", dict(group_films=True, albedo=bad), "albedo [H,W,4] of the film's size")):
        with pytest.raises(ValueError) as e:
            getattr(lib, method)(**filter_inputs(**inputs))
        assert str(e.value) == message, method
    with pytest.raises(api.PtError, match="denoise_spectral takes no albedo"):
        lib.denoise_spectral(albedo=bad, **filter_inputs(spectral=True))
    assert fake.entries() == []


# ---- the resident methods -------------------------------------------------------------------------------------------------------------------------------
RESIDENT = "resident_last_error"
LG, LGS = "light_groups_last_error", "light_groups_spectral_last_error"
M_KB, M_G33, M_KGB = np.zeros((4, BINS), np.float32), np.zeros((G, 3, 3), np.float32), np.zeros((4, G, BINS), np.float32)
# case -> (the call, the entries it reaches in order, the last one's emulation error channel, what comes back)
RESIDENTS = {
    "resident_info": (lambda s: s.resident_info(), ["resident_info"], RESIDENT, (W, H, BINS, 0)),
    "resident_guides": (lambda s: s.resident_guides(s.rd, 4, 0, albedo=True), ["resident_guides"], RESIDENT, None),
    "resident_load": (lambda s: s.resident_load(guides=np.zeros((H, W, 4), np.float32)), ["resident_load"], RESIDENT, None),
    "resident_assemble": (lambda s: s.resident_assemble(), ["resident_assemble"], RESIDENT, None),
    "resident_read": (lambda s: s.resident_read(spectral=True), ["resident_info", "resident_read"], RESIDENT, ["film", "counts", "stats", "spectral"]),
    "resident_read_one": (lambda s: s.resident_read(film=False, stats=False), ["resident_info", "resident_read"], RESIDENT, "counts"),
    "resident_read_none": (lambda s: s.resident_read(False, False, False), ["resident_info", "resident_read"], RESIDENT, None),
    "denoise_resident": (lambda s: s.denoise_resident(variance=True, spectral=True), ["resident_info", "denoise_resident"], RESIDENT, ["film", "variance", "spectral"]),
    "denoise_resident_one": (lambda s: s.denoise_resident(), ["resident_info", "denoise_resident"], RESIDENT, "film"),
    "spectral_project_resident": (lambda s: s.spectral_project_resident(M_KB), ["spectral_resident", "spectral_project_resident"], None, (4, H, W)),
    "spectral_project_resident_denoised": (lambda s: s.spectral_project_resident(M_KB, denoised=True), ["resident_info", "spectral_project_resident_denoised"], RESIDENT,
                                           (4, H, W)),
    "spectral_resident": (lambda s: s.spectral_resident(), ["spectral_resident"], None, (W, H, BINS)),
    "light_groups_resident": (lambda s: s.light_groups_resident(), ["light_groups_resident"], LG, (W, H, G)),
    "light_groups_spectral_resident": (lambda s: s.light_groups_spectral_resident(), ["light_groups_spectral_resident"], LGS, (W, H, G, BINS)),
    "light_groups_denoised_resident": (lambda s: s.light_groups_denoised_resident(), ["light_groups_denoised_resident"], None, (W, H, G)),
    "light_groups_mix_resident": (lambda s: s.light_groups_mix_resident(M_G33), ["light_groups_resident", "light_groups_mix_resident"], LG, (H, W, 4)),
    "light_groups_mix_resident_denoised": (lambda s: s.light_groups_mix_resident(M_G33, denoised=True),
                                           ["light_groups_denoised_resident", "light_groups_mix_resident_denoised"], LG, (H, W, 4)),
    "light_groups_relamp_resident": (lambda s: s.light_groups_relamp_resident(M_KGB), ["light_groups_spectral_resident", "light_groups_relamp_resident"], LGS, (4, H, W)),
    "denoise_light_groups_resident": (lambda s: s.denoise_light_groups_resident(variance=True), ["resident_info", "light_groups_resident", "denoise_light_groups_resident"],
                                      None, ["film", "variance", "group_films"]),
    "denoise_light_groups_resident_one": (lambda s: s.denoise_light_groups_resident(film=False, groups=False, variance=True),
                                          ["resident_info", "light_groups_resident", "denoise_light_groups_resident"], None, "variance"),
}


@pytest.mark.parametrize("case", sorted(RESIDENTS))
def test_resident_method(make, case):
    call, entries, channel, want = RESIDENTS[case]
    api, fake, lib, scene = make()
    scene.rd = api.render_desc(W, H, 1, 2)
    got = call(scene)
    assert fake.entries() == entries
    for name, args in fake.calls:
        assert len(args) == len(getattr(lib, "_" + name).argtypes), name
        assert args[0] is scene.handle
    if isinstance(want, list):
        assert isinstance(got, tuple) and len(got) == len(want)
        for a, kind in zip(got, want):
            check_array(a, kind, case)
    elif isinstance(want, str):
        check_array(got, want, case)
    elif isinstance(got, np.ndarray):
        assert got.shape == want and got.dtype == np.float32
    else:
        assert got == want
    # the outputs not asked for are None, the others point at what came back
    outs = fake.calls[-1][1]
    if case.startswith("resident_read"):
        asked = {"resident_read": (1, 1, 1, 1), "resident_read_one": (0, 1, 0, 0), "resident_read_none": (0, 0, 0, 0)}[case]
        assert [a is not None for a in outs[1:]] == [bool(x) for x in asked]
    if case.startswith("denoise_resident") or case.startswith("denoise_light_groups_resident"):
        asked = {"denoise_resident": (1, 1, 1), "denoise_resident_one": (1, 0, 0), "denoise_light_groups_resident": (1, 1, 1),
                 "denoise_light_groups_resident_one": (0, 1, 0)}[case]
        assert [a is not None for a in outs[2:]] == [bool(x) for x in asked]
        assert isinstance(outs[1]._obj, api.ResidentDenoiseDesc)

    def again(api, lib, scene):
        scene.rd = api.render_desc(W, H, 1, 2)
        return call(scene)
    expect_refusals(make, again, entries[-1], channel)


def test_resident_queries_answer_none_for_an_empty_scene(make, monkeypatch):
    api, fake, lib, scene = make()
    monkeypatch.setattr(FakeFn, "__call__", lambda self, *args: self.lib.calls.append((self.name, args)) or 0)
    for query in ("spectral_resident", "light_groups_resident", "light_groups_spectral_resident", "light_groups_denoised_resident"):
        assert getattr(scene, query)() is None
    with pytest.raises(api.PtError, match="pt_status 1: the scene has no resident group films"):
        scene.light_groups_mix_resident(M_G33)
    with pytest.raises(api.PtError, match="pt_status 1: the scene has no resident denoised group films"):
        scene.light_groups_mix_resident(M_G33, denoised=True)


def test_resident_load_hands_over_what_is_given(make):
    api, fake, lib, scene = make()
    z = lambda kind: np.zeros(*SHAPES[kind])
    film, counts, stats, spectral = z("film"), z("counts"), z("stats"), z("spectral")
    scene.resident_load(film=film, counts=counts, stats=stats, spectral=spectral)
    args = fake.calls[0][1]
    assert args[1:4] == (W, H, BINS)
    assert [address(a) if a is not None else None for a in args[4:]] == [film.ctypes.data, counts.ctypes.data, stats.ctypes.data, spectral.ctypes.data, None, None, None]
    with pytest.raises(ValueError, match="of one size"):
        scene.resident_load(film=film, guides=np.zeros((H + 1, W, 4), np.float32))
    with pytest.raises(ValueError, match=r"film, guides and albedo \[H,W,4\], stats \[H,W,2\]"):
        scene.resident_load(film=np.zeros((H, W, 3), np.float32))


# ---- the guide renders and the other entries with a channel of their own --------------------------------------------------------------------------------
OTHERS = {
    "render_guides": (lambda a, l, s: s.render_guides(s.rd), "denoise_last_error"),
    "render_guides_albedo": (lambda a, l, s: s.render_guides_albedo(s.rd), "denoise_albedo_last_error"),
    "render_guides_chain": (lambda a, l, s: s.render_guides_chain(s.rd), "guides_chain_last_error"),
    "render_guides_bin_albedo": (lambda a, l, s: s.render_guides_bin_albedo(s.rd, BINS), "denoise_spectral_albedo_last_error"),
    "albedo_basis": (lambda a, l, s: l.albedo_basis(s.rd), "denoise_albedo_last_error"),
    "spectral_bin_centres": (lambda a, l, s: l.spectral_bin_centres(s.rd, BINS), None),
    "write_exr_spectral": (lambda a, l, s: l.write_exr_spectral("x.exr", np.zeros(BINS), np.zeros((BINS, H, W))), None),
    "spectral_response_matrix": (lambda a, l, s: l.spectral_observer_matrix(s.rd, BINS), "spectral_project_last_error"),
    "spectral_project": (lambda a, l, s: l.spectral_project(np.zeros((BINS, H, W)), M_KB), "spectral_project_last_error"),
    "light_groups_mix": (lambda a, l, s: l.light_groups_mix(np.zeros((G, H, W, 4)), M_G33), LG),
    "light_groups_relamp_matrix": (lambda a, l, s: l.light_groups_relamp_matrix(s.rd, BINS, (a.RESPONSE_CIE_Y,), G, [None] * G, [None] * G, gain=[1.0] * G), LGS),
    "light_groups_relamp": (lambda a, l, s: l.light_groups_relamp(np.zeros((G, BINS, H, W)), M_KGB), LGS),
}


@pytest.mark.parametrize("entry", sorted(OTHERS))
def test_other_entry(make, entry):
    call, channel = OTHERS[entry]

    def run(api, lib, scene):
        scene.rd = api.render_desc(W, H, 1, 2)
        return call(api, lib, scene)
    api, fake, lib, scene = make()
    got = run(api, lib, scene)
    assert fake.entries() == [entry]
    assert len(fake.calls[0][1]) == len(getattr(lib, "_" + entry).argtypes)
    shapes = [a.shape for a in (got if isinstance(got, tuple) else (got,)) if a is not None]
    assert shapes == {"render_guides": [(H, W, 4)], "render_guides_albedo": [(H, W, 4)] * 2, "render_guides_chain": [(H, W, 4)] * 2,
                      "render_guides_bin_albedo": [(H, W, 4), (H, W, 4), (BINS, H, W)], "albedo_basis": [(16,), (3, 16)], "spectral_bin_centres": [(BINS,)],
                      "write_exr_spectral": [], "spectral_response_matrix": [(3, BINS)], "spectral_project": [(4, H, W)], "light_groups_mix": [(H, W, 4)],
                      "light_groups_relamp_matrix": [(1, G, BINS)], "light_groups_relamp": [(4, H, W)]}[entry]
    expect_refusals(make, run, entry, channel)


def test_guides_without_an_albedo_or_a_chain_pass_none(make):
    api, fake, lib, scene = make()
    rd = api.render_desc(W, H, 1, 2)
    g, a = scene.render_guides_chain(rd, albedo=False)
    assert a is None and fake.calls[-1][1][-1] is None and fake.calls[-1][1][3]._obj.max_chain == 8
    scene.render_guides_bin_albedo(rd, BINS)
    assert fake.calls[-1][1][3] is None
    scene.render_guides_bin_albedo(rd, BINS, max_chain=2)
    assert fake.calls[-1][1][3]._obj.max_chain == 2
    scene.resident_guides(rd)
    assert fake.calls[-1][1][2:] == (4, None, 0)
    scene.resident_guides(rd, 2, 3, albedo=True, bin_albedo=True)
    assert fake.calls[-1][1][3]._obj.max_chain == 3 and fake.calls[-1][1][4] == api.RESIDENT_ALBEDO | api.RESIDENT_BIN_ALBEDO


def test_binding_semantics(make, pkg, monkeypatch):
    """A missing required entry refuses the load unless `optional` names it; any other missing entry is None; the two tuning refusals keep their wording."""
    api = pkg.api
    with pytest.raises(AttributeError):
        make(("intersect",))
    fake = FakeLib()
    fake.missing = {"intersect", "render_spectral", "scene_create_tuned", "tuning_default"}
    monkeypatch.setattr(C, "CDLL", lambda path: fake)
    lib = api.Library(PATH, "pt_", optional=("intersect",))
    assert lib._intersect is None and lib._render_spectral is None and lib._render is fake.pt_render
    assert lib._render.restype is C.c_int32 and lib._last_error.restype is C.c_char_p and len(lib._render.argtypes) == 4
    with pytest.raises(api.PtError, match="pt_status 4: this library does not export pt_tuning_default \\(pt_tuning is the HIP engine's\\)"):
        lib.tuning_default()
    with pytest.raises(api.PtError, match="pt_status 4: this library does not export pt_scene_create_tuned \\(pt_tuning is the HIP engine's\\)"):
        lib.create_scene(Builder(api), tuning=api.Tuning())
    fake.fail["scene_create"] = 1
    with pytest.raises(api.PtError, match="pt_status 1: last_error$"):
        lib.create_scene(Builder(api))
    assert lib.device_info() == "device_info"
    fake.missing.add("device_info")
    assert api.Library(PATH, "pt_", optional=("intersect",)).device_info() == "cpu oracle"


# ---- the three composites -------------------------------------------------------------------------------------------------------------------------------
INFO, GUIDES_RES = "resident_info", "resident_guides"
DEN_RES = [INFO, "denoise_resident"]
DEN_LG_RES = [INFO, "light_groups_resident", "denoise_light_groups_resident"]
# (method, keywords, resident parts the fake reports) -> the entries reached, in order
COMPOSITES = [
    ("render_denoised", {}, 0, ["render_adaptive", "render_guides", "denoise_film"]),
    ("render_denoised", dict(albedo=True), 0, ["render_adaptive", "render_guides_albedo", "denoise_film_albedo"]),
    ("render_denoised", dict(specular_chain=0), 0, ["render_adaptive", "render_guides_chain", "denoise_film"]),
    ("render_denoised", dict(specular_chain=2, albedo=True), 0, ["render_adaptive", "render_guides_chain", "denoise_film_albedo"]),
    ("render_denoised", dict(device_mask=MASK), 0, ["render_adaptive_multi", "render_guides", "denoise_film"]),
    ("render_denoised", dict(resident=True, albedo=True), 0, ["render_adaptive", GUIDES_RES] + DEN_RES),
    ("render_denoised", dict(assemble=True, device_mask=MASK), 0, ["render_adaptive_multi", INFO, "resident_assemble", GUIDES_RES] + DEN_RES),
    ("render_denoised", dict(assemble=True, device_mask=MASK), 1, ["render_adaptive_multi", INFO, GUIDES_RES] + DEN_RES),
    ("render_denoised_spectral", {}, 0, ["render_adaptive_spectral", "render_guides", "denoise_spectral"]),
    ("render_denoised_spectral", dict(specular_chain=2), 0, ["render_adaptive_spectral", "render_guides_chain", "denoise_spectral"]),
    ("render_denoised_spectral", dict(bin_albedo=True), 0, ["render_adaptive_spectral", "render_guides_bin_albedo", "denoise_spectral_albedo"]),
    ("render_denoised_spectral", dict(device_mask=MASK), 0, ["render_adaptive_spectral_multi", "render_guides", "denoise_spectral"]),
    ("render_denoised_spectral", dict(device_mask=MASK, bin_albedo=True), 0, ["render_adaptive_spectral_multi", "render_guides_bin_albedo", "denoise_spectral_albedo"]),
    ("render_denoised_spectral", dict(resident=True, bin_albedo=True), 0, ["render_adaptive_spectral", GUIDES_RES] + DEN_RES),
    ("render_denoised_spectral", dict(assemble=True, device_mask=MASK), 0, ["render_adaptive_spectral_multi", INFO, "resident_assemble", GUIDES_RES] + DEN_RES),
    ("render_denoised_spectral", dict(assemble=True, device_mask=MASK), 1, ["render_adaptive_spectral_multi", INFO, GUIDES_RES] + DEN_RES),
    ("render_denoised_light_groups", {}, 0, ["render_adaptive_light_groups", GUIDES_RES] + DEN_LG_RES),
    ("render_denoised_light_groups", dict(device_mask=MASK), 0, ["render_adaptive_light_groups_multi", INFO, "render_guides", "denoise_light_groups"]),
    ("render_denoised_light_groups", dict(device_mask=MASK, albedo=True), 0, ["render_adaptive_light_groups_multi", INFO, "render_guides_albedo", "denoise_light_groups"]),
    ("render_denoised_light_groups", dict(device_mask=MASK, specular_chain=2), 0,
     ["render_adaptive_light_groups_multi", INFO, "render_guides_chain", "denoise_light_groups"]),
    ("render_denoised_light_groups", dict(device_mask=MASK), 1, ["render_adaptive_light_groups_multi", INFO, GUIDES_RES] + DEN_LG_RES),
    ("render_denoised_light_groups", dict(device_mask=MASK, assemble=True), 0,
     ["render_adaptive_light_groups_multi", INFO, "resident_assemble", GUIDES_RES] + DEN_LG_RES),
    ("render_denoised_light_groups", dict(device_mask=MASK, assemble=True), 1, ["render_adaptive_light_groups_multi", INFO, GUIDES_RES] + DEN_LG_RES),
]
COMPOSITE_ARGS = {"render_denoised": {}, "render_denoised_spectral": dict(bins=BINS), "render_denoised_light_groups": dict(instance_group=IDS)}
COMPOSITE_RETURNS = {"render_denoised": ["film", "film", "counts"], "render_denoised_spectral": ["film", "film", "spectral", "spectral", "counts"],
                     "render_denoised_light_groups": ["film", "film", "group_films", "group_films", "counts"]}


@pytest.mark.parametrize("index", range(len(COMPOSITES)))
def test_composite_route(make, index):
    method, kw, parts, entries = COMPOSITES[index]
    api, fake, lib, scene = make()
    fake.parts = parts
    rd = api.render_desc(W, H, 3, 2)
    got = getattr(scene, method)(rd, guide_samples=2, iterations=3, **dict(COMPOSITE_ARGS[method], **kw))
    assert fake.entries() == entries
    for name, args in fake.calls:
        assert len(args) == len(getattr(lib, "_" + name).argtypes), name
    want = COMPOSITE_RETURNS[method]
    assert isinstance(got, tuple) and len(got) == len(want) + 1 and isinstance(got[-1], api.Profile)
    for a, kind in zip(got, want):
        check_array(a, kind, (method, kw))
    calls = dict(fake.calls)
    render = calls[entries[0]]
    ad = next(a._obj for a in render if isinstance(getattr(a, "_obj", None), api.AdaptiveDesc))
    assert ad.max_samples == 3   # (max_samples None: rd.spp)
    assert sum(a is None for a in render) == 0   # (the statistics are always asked for)
    if GUIDES_RES in calls:
        chain, flags = calls[GUIDES_RES][3:]
        want_chain = kw.get("specular_chain") or 0
        assert (chain._obj.max_chain if want_chain else chain) == (want_chain or None) and calls[GUIDES_RES][2] == 2
        assert flags == (api.RESIDENT_ALBEDO if kw.get("albedo") else 0) | (api.RESIDENT_ALBEDO | api.RESIDENT_BIN_ALBEDO if kw.get("bin_albedo") else 0)
    else:
        d = calls[entries[-1]][0]._obj
        assert (d.width, d.height, d.iterations, d.device) == (W, H, 3, 0)   # (the first device of 0b101)


def test_composite_filters_on_the_first_device_of_the_mask(make):
    api, fake, lib, scene = make()
    rd = api.render_desc(W, H, 3, 2)
    for mask, first in ((0b100, 2), (0b110, 1), (0, 0), (1 << 40, 40)):
        for method in COMPOSITE_ARGS:
            getattr(scene, method)(rd, device_mask=mask, **COMPOSITE_ARGS[method])
            assert fake.calls[-1][1][0]._obj.device == first, (method, mask)
            mask_arg = next(a for n, a in fake.calls if n.endswith("_multi"))[3 if method == "render_denoised" else 4]
            assert getattr(mask_arg, "value", mask_arg) == mask
            fake.calls.clear()


def test_composite_refusals(make):
    api, fake, lib, scene = make()
    rd = api.render_desc(W, H, 3, 2)
    for method in ("render_denoised", "render_denoised_spectral"):
        with pytest.raises(api.PtError, match="pt_status 4: %s: assemble=True needs a device_mask" % method):
            getattr(scene, method)(rd, assemble=True, **COMPOSITE_ARGS[method])
        with pytest.raises(api.PtError, match="pt_status 4: %s: resident=True takes no device_mask" % method):
            getattr(scene, method)(rd, resident=True, device_mask=1, **COMPOSITE_ARGS[method])
    with pytest.raises(api.PtError, match="pt_status 4: render_denoised_spectral takes no albedo"):
        scene.render_denoised_spectral(rd, BINS, albedo=True)
    with pytest.raises(ValueError, match="assemble gathers a node render: it needs a device_mask"):
        scene.render_denoised_light_groups(rd, IDS, assemble=True)
    assert fake.entries() == []
