"""Path expressions (include/pt_light_groups.h "Path expressions"): films for user-written light-path patterns — a small automaton over the
path's scattering events with the emitter as the last symbol, compiled on the host (csrc/pt_path_expr.cpp) and run by the third router of the routed render
(ExprRouter, csrc/pt_path_expr_rules.h).

The CPU tier checks the compiler against Python's `re` over every short path; the host emulation (tests/host_emulation/ptemu_path_exprs.cpp: the routed render's
pass loop, ptemu_routed_pass.h, under the engine's ExprRouter) against the two routers the expressions subsume — the path passes and the light groups, per plane
with numpy.array_equal — against ptemu_render, against itself with other expressions compiled beside (independence) and against a third reading in scalar Python
laid over tests/test_integrator_third_reading.py's vertex list; then the refusals, the header, the binding rows, the command line and the sanitizer program.  The
GPU tier checks the engine against the emulation bit for bit and against its own other entries."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import emulation
import test_integrator_third_reading as t3
import test_path_passes as tpp
from util import ptcli, same_bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
CSRC = os.path.join(ROOT, "rust-pathtracer_amd", "csrc")
f32 = np.float32
F = np.float32

# the emulation library of this file: ptemu.cpp, the expression render and the product's own compiler
EMU_TABLE = {"path_exprs": "ptemu.cpp ptemu_path_exprs.cpp pt_path_expr.cpp" + emulation.HOST}

BUILT_IN = ("CL", "CE", "CD[LE]", "CD.+[LE]", "CR[LE]", "CR.+[LE]", "CT[LE]", "CT.+[LE]")   # the eight path passes, in the order of PT_PATH_PASS_*
# expressions that overlap and nest: everything; caustics; a grouped alternation with a labelled lamp beside a top-level alternative; the sky seen without a
# diffuse event; everything that passed through glass at least twice
OVERLAP = ("C.*[LE]", "CD[RT]+[LE]", "C(DR|T?D)*L1|CR+E", "C[^D]*E0", "C.*T.*T.*[LE]")
# scene.path_passes_room: instance 1 is the rect lamp, instance 2 the disk lamp, each a light group of its own; the environment is in group 0
PANE_GROUPS, PANE_ENV_GROUP = (0, 1, 2, 0, 0, 0, 0), 0
ROOM_GROUPS, ROOM_ENV_GROUP = (0, 0, 1, 0, 0, 0), 2   # tests/test_light_groups.py's


def counters(p):
    return (p.camera_rays, p.bounce_rays, p.shadow_rays, p.env_hits)


def pane_rd(pkg, light_samples=2):
    """The GPU tier's case: a film that is no multiple of a wave or a tile, 8 spp, 5 bounces."""
    return pkg.api.render_desc(24, 16, 8, 5, light_samples=light_samples, seed=7)


@pytest.fixture(scope="session")
def emu_px(pkg):
    """The host emulation (ptemu.cpp) with the expression render (ptemu_path_exprs.cpp) and the compiler beside it: a library of its own."""
    return pkg.api.Library(emulation.library_path("path_exprs", table=EMU_TABLE), "ptemu_", optional=("render_device", "device_info"))


@pytest.fixture(scope="session")
def emu_pp(pkg):
    return emulation.load(pkg, "path_passes")


@pytest.fixture(scope="session")
def emu_lg(pkg):
    return emulation.load(pkg, "light_groups")


@pytest.fixture(scope="session")
def pane_emu(pkg, emu_px):
    """The emulation's renders of the room behind the pane with the five overlapping expressions, made once and left unchanged: light_samples 2 and 3."""
    out = {}
    for L in (2, 3):
        film, films, prof = emu_px.create_scene(pkg.scene.path_passes_room()).render_path_exprs(pane_rd(pkg, L), OVERLAP, PANE_GROUPS, PANE_ENV_GROUP)
        film.setflags(write=False); films.setflags(write=False)
        out[L] = {"film": film, "films": films, "prof": prof}
    return out


# ------------------------------------------------------------------------------------------------ the compiler
def to_re(expr, environment_group):
    """A second reading of the language: the expression as a Python `re` over one character per symbol — C, the events D R T, the surface emitter of group g as the
    digit g, the environment as e."""
    text, out, i = re.sub(r"\s", "", expr), [], 0

    def terminal(i):
        """(characters, next index) of L, L<g>, E, E<g> at i"""
        digit = text[i + 1] if i + 1 < len(text) and text[i + 1].isdigit() else None
        if text[i] == "L":
            chars = "01234567" if digit is None else digit
        else:
            chars = "e" if digit is None or int(digit) == environment_group else ""
        return chars, i + (1 if digit is None else 2)
    while i < len(text):
        c = text[i]
        if c in "CDRT()|*+?":
            out.append(c); i += 1
        elif c == ".":
            out.append("[DRT]"); i += 1
        elif c in "LE":
            chars, i = terminal(i)
            out.append("[%s]" % chars if chars else "(?!)")
        elif c == "[":
            close = text.index("]", i)
            body = text[i + 1:close]
            if body[0] == "^":
                out.append("[%s]" % "".join(sorted(set("DRT") - set(body[1:]))))
            elif body[0] in "DRT":
                assert set(body) <= set("DRT")
                out.append("[%s]" % body)
            else:
                chars, j = "", i + 1
                while j < close:
                    more, j = terminal(j)
                    chars += more
                out.append("[%s]" % chars if chars else "(?!)")
            i = close + 1
        else:
            raise AssertionError("to_re: %r in %r" % (c, expr))
    return re.compile("".join(out))


def every_short_path():
    """(the path as pt_path_expr_match takes it, the same path one character per symbol): C, up to 6 events, each of the 9 terminals — 9 * (3^7 - 1) / 2 = 9837."""
    for n in range(7):
        for events in itertools.product("DRT", repeat=n):
            for t in range(9):
                yield "C" + "".join(events) + ("L%d" % t if t < 8 else "E"), "C" + "".join(events) + ("%d" % t if t < 8 else "e")


@pytest.mark.parametrize("exprs,env,empty", [(BUILT_IN, 0, ()), (OVERLAP, 0, ()), (OVERLAP, 3, (3,)),
                                             (("C.*[L2E2]", "C (D | R)* T+ [E1 L7 L0]", "C(D(R(T)?)*)+E|CL3|C.?.?L", "C[^DR][^T]*L"), 2, ())],
                         ids=["built-in", "overlap", "overlap-env3", "classes-env2"])
def test_compiler_agrees_with_re(pkg, exprs, env, empty):
    """pt_path_expr_match's mask over every path of up to 6 events equals the set of expressions whose `re` fully matches.  empty: the expressions that match
    no path at all (C[^D]*E0 where the environment is in group 3)."""
    lib = pkg.load()
    program = lib.path_expr_compile(exprs, env)
    assert program.outputs == len(exprs) and 1 <= program.states <= 64 and program.start < program.states and program.environment_group == env
    regexes = [to_re(e, env) for e in exprs]
    n, hits = 0, [0] * len(exprs)
    for path, chars in every_short_path():
        want = sum(1 << e for e, r in enumerate(regexes) if r.fullmatch(chars))
        assert lib.path_expr_match(program, path) == want, (path, want)
        n += 1
        for e in range(len(exprs)):
            hits[e] += (want >> e) & 1
    print("states %d; paths %d; matched per expression %s" % (program.states, n, hits))
    assert n == 9837 and [e for e, h in enumerate(hits) if not h] == list(empty)


def test_program_layout(pkg):
    """The table as the header documents it: successors in word 0, nine byte masks in words 1..3, zero beyond `states`; L sets all eight surface symbols, E<g> of
    another group than the environment's sets none; the state nothing is accepted from is an ordinary state with zero masks."""
    lib = pkg.load()
    p = lib.path_expr_compile(["CDL", "CE5", "CDE2"], 2)
    table = np.ctypeslib.as_array(p.table).reshape(64, 4)
    assert not table[p.states:].any() and (table[:p.states, 0] >> 18 == 0).all()

    def step(q, event):
        return int(table[q, 0] >> (6 * "DRT".index(event))) & 63

    def mask(q, t):
        return int(table[q, 1 + t // 4] >> (8 * (t % 4))) & 0xff
    start, d = p.start, step(p.start, "D")
    assert [mask(start, t) for t in range(9)] == [0] * 9          # (CE5: the environment is in group 2)
    assert [mask(d, t) for t in range(9)] == [1] * 8 + [4]        # CDL: every surface group; CDE2: the environment
    dead = step(d, "D")
    assert all(step(dead, e) == dead for e in "DRT") and not table[dead, 1:].any() and step(start, "T") == dead
    assert lib.path_expr_match(p, "CDL") == 1 and lib.path_expr_match(p, "CDL6") == 1 and lib.path_expr_match(p, "CDE") == 4 and lib.path_expr_match(p, "CE") == 0
    for bad in ("", "DL", "CDX", "CD", "CDL8", "CDLL", "C D L"):
        with pytest.raises(pkg.api.PtError) as e:
            lib.path_expr_match(p, bad)
        assert e.value.status == pkg.api.PT_ERR_INVALID_ARGUMENT


SYNTAX_ERRORS = [
    ("DL", 1, "starts with C"), ("", 1, "starts with C"), ("  ", 3, "starts with C"), ("CD", 3, "without a terminal"), ("CD(", 4, "')' expected"),
    ("CD)L", 3, "closes no group"), ("C(DL)", 4, "terminal inside a group"), ("C*L", 2, "follows no event"), ("CD|RL", 3, "terminal"), ("CDxL", 3, "'x'"),
    ("CDL9", 4, "0..7"), ("CDLD", 4, "only '|'"), ("CDL|", 5, "starts with C"), ("C[DX]L", 4, "class of events"), ("C[^DRT]L", 7, "empty"), ("C[D", 4, "not closed"),
    ("CD[LD]", 5, "class of terminals"), ("C()L", 3, "empty group"), ("C(D|R L", 7, "terminal inside a group"), ("CCL", 2, "only at the start"), ("C D  ?? x", 9, "'x'"),
    ("C(D", 4, "')' expected"),
]


@pytest.mark.parametrize("text,column,word", SYNTAX_ERRORS, ids=[repr(s[0]) for s in SYNTAX_ERRORS])
def test_syntax_errors_name_their_column(pkg, text, column, word):
    """Anything outside the language is PT_ERR_INVALID_ARGUMENT, reported with the expression's index and the column, counted from 1 in the text as given."""
    with pytest.raises(pkg.api.PtError) as e:
        pkg.load().path_expr_compile(["CL", text])
    print(str(e.value))
    assert e.value.status == pkg.api.PT_ERR_INVALID_ARGUMENT and ("expression 1, column %d: " % column) in str(e.value) and word in str(e.value), str(e.value)


def test_compile_refusals(pkg):
    """More than 64 states is PT_ERR_UNSUPPORTED and names the count.  "The seventh event from the end is diffuse" needs the D-ness of the last seven events:
    2^7 = 128 states, none of which another can stand for.  Also: the number of expressions, the environment's group, a null."""
    a, lib = pkg.api, pkg.load()
    with pytest.raises(a.PtError) as e:
        lib.path_expr_compile("C.*D......L")
    print(str(e.value))
    assert e.value.status == a.PT_ERR_UNSUPPORTED and "128 states" in str(e.value) and "at most 64" in str(e.value)
    assert lib.path_expr_compile("C.*D.....L").states == 64   # (one event fewer: 2^6, the largest program)
    for exprs, env, word in (([], 0, "1..8"), (["CL"] * 9, 0, "1..8"), (["CL"], 8, "environment_group")):
        with pytest.raises(a.PtError) as e:
            lib.path_expr_compile(exprs, env)
        assert e.value.status == a.PT_ERR_INVALID_ARGUMENT and word in str(e.value)
    err = C.create_string_buffer(64)
    assert lib._path_expr_compile(None, 1, 0, C.byref(a.PathExprProgram()), err, 64) == a.PT_ERR_INVALID_ARGUMENT and b"null" in err.value
    short = C.create_string_buffer(8)   # (the message is cut to the buffer and terminated)
    texts = (C.c_char_p * 1)(b"CD")
    assert lib._path_expr_compile(texts, 1, 0, C.byref(a.PathExprProgram()), short, 8) == a.PT_ERR_INVALID_ARGUMENT and short.value == b"express"


# ------------------------------------------------------------------------------------------------ the emulation
def planes_equal(got, want, names):
    """numpy.array_equal per plane: a signed zero passes, nothing else."""
    assert got.shape == want.shape
    for c, name in enumerate(names):
        assert np.array_equal(got[c], want[c]), name


@pytest.mark.parametrize("which", ["pane", "cornell"])
def test_built_in_expressions_are_the_path_passes(pkg, emu_px, emu_pp, which):
    """The eight built-in expressions give the eight films of the path-pass emulation, on the room behind the pane (all eight lit) and on the Cornell box."""
    if which == "pane":
        scene, rd = pkg.scene.path_passes_room(), tpp.room_rd(pkg)
    else:
        scene, rd = pkg.scene.cornell_box(), pkg.api.render_desc(16, 16, 12, 5, light_samples=2, seed=3)
    film, films, prof = emu_px.create_scene(scene).render_path_exprs(rd, pkg.api.PATH_PASS_EXPRS)
    wfilm, passes, wprof = emu_pp.create_scene(scene).render_path_passes(rd)
    assert tuple(pkg.api.PATH_PASS_EXPRS) == BUILT_IN
    assert same_bits(film, wfilm) and counters(prof) == counters(wprof)
    planes_equal(films, passes, tpp.NAMES)
    lit = [c for c in range(8) if passes[c][..., :3].any()]
    assert lit == (list(range(8)) if which == "pane" else [0, 2, 3])


def group_exprs(G):
    return ["C.*[L%dE%d]" % (g, g) for g in range(G)]


def test_group_expressions_are_the_light_groups(pkg, emu_px, emu_lg):
    """C.*[LgEg] for g = 0..G-1 gives light_groups_room's group films."""
    rd = tpp.room_rd(pkg)
    room = pkg.scene.light_groups_room()
    film, films, prof = emu_px.create_scene(room).render_path_exprs(rd, group_exprs(3), ROOM_GROUPS, ROOM_ENV_GROUP)
    wfilm, groups, wprof = emu_lg.create_scene(room).render_light_groups(rd, ROOM_GROUPS, ROOM_ENV_GROUP)
    assert same_bits(film, wfilm) and counters(prof) == counters(wprof)
    planes_equal(films, groups, ("rect lamp", "disk lamp", "sky"))
    assert all(groups[g][..., :3].any() for g in range(3))


def test_everything_is_the_film(pkg, emu_px, monkeypatch):
    """C.*[LE] alone gives the XYZ of the total film bit for bit; total film and ray counters equal ptemu_render's, also when cut into passes."""
    rd = tpp.room_rd(pkg)
    pane = pkg.scene.path_passes_room()
    plain, pprof = emu_px.create_scene(pane).render(rd)
    film, films, prof = emu_px.create_scene(pane).render_path_exprs(rd, "C.*[LE]", PANE_GROUPS)
    assert same_bits(film, plain) and counters(prof) == counters(pprof)
    assert films.shape == (1, 24, 24, 4) and same_bits(films[0][..., :3], plain[..., :3]) and not films[..., 3].any()
    monkeypatch.setenv("PTEMU_BATCH", "2048")   # (24 x 24 x 23 = 13248 slots: at least seven passes)
    film2, films2, prof2 = emu_px.create_scene(pane).render_path_exprs(rd, "C.*[LE]", PANE_GROUPS)
    assert same_bits(film2, plain) and same_bits(films2, films) and counters(prof2) == counters(pprof)


@pytest.mark.parametrize("L", [2, 3])
def test_an_expressions_film_does_not_depend_on_the_set(pkg, emu_px, pane_emu, L):
    """Each of the five overlapping expressions' films equals its film rendered alone, bit for bit; all five are lit and the four proper ones differ from the total."""
    e = pane_emu[L]
    for k, expr in enumerate(OVERLAP):
        film, alone, prof = emu_px.create_scene(pkg.scene.path_passes_room()).render_path_exprs(pane_rd(pkg, L), expr, PANE_GROUPS, PANE_ENV_GROUP)
        assert same_bits(film, e["film"]) and counters(prof) == counters(e["prof"])
        assert same_bits(alone[0], e["films"][k]), expr
        lit = int((alone[0][..., :3] != 0).any(axis=-1).sum())
        print("%-22s lit pixels %4d  max %.4g" % (expr, lit, float(alone[0][..., :3].max())))
        assert lit > 0 and np.isfinite(alone).all() and not alone[..., 3].any()
        assert k == 0 or not same_bits(alone[0], e["films"][0])
    assert same_bits(e["films"][0][..., :3], e["film"][..., :3])


# ---- a third reading: scalar Python over test_integrator_third_reading.py's vertex list, every contribution's path written out and matched with `re`
def lamps_behind_a_pane(pkg):
    """t3.sky_and_lamp — a lamp, a white and a rough-glass sphere over a floor under a sampled sky — with a second lamp and, between the camera and the half of it
    that holds that lamp, a pane of rough glass (the glass sphere and its caustics are seen beside the pane): the room behind the pane as the third reading can read it (its light sampling knows one-sided +Z rects alone, and scene.path_passes_room's
    second lamp is a disk)."""
    b = t3.sky_and_lamp(pkg)
    b.add_rect((0.4, 0.4), (0.3, 1.1, 0.0), "Z", False, pkg.scene.add_library_material(b, "diffuse_light_flat_x5"))
    b.add_rect((1.6, 1.6), (-1.8, 0.8, 0.9), "X", True, pkg.scene.add_library_material(b, "ggx_glass_rough"))
    return b


def third_light_samples(P, lights, groups, lam, v, n, frame, wi, pixel, sample, bounce, path, regexes, energy):
    """t3.direct_illumination per ray: a ray continues the path by the event of its own direction and ends on the lamp it hit (or on the sky); each expression's
    matching rays are summed in ray order and divided by light_samples once."""
    rd = P.rd
    sums = {}
    env_p = F(P.b.env_sampling_probability) if lights else F(1.0)
    for l in range(rd.light_samples):
        r = P.draw4(pixel, sample, 32 + bounce * (1 + rd.light_samples) + 1 + l)
        x = r[0]
        if x < env_p:
            direction = t3.uv_to_direction(P, r[1], r[2])
            c = t3.direct_illumination_from_world(P, lam, v.point, n, frame, wi, v.material, v.throughput, r[1:3])
            terminal = "e"
        else:
            x = F(F(x - env_p) / F(F(1.0) - env_p))
            cnt = len(lights)
            idx = int(min(max(F(F(cnt) * x), F(0.0)), F(cnt - 1)))
            direction, light_pdf = t3.rect_sample(lights[idx][1], r[1:3], v.point)
            light_pdf = F(light_pdf * F(F(1.0) / F(cnt)))
            if light_pdf == 0:
                continue
            wo = frame.to_local(direction)
            refl, bounce_pdf = P.bsdf(v.material, lam, wi, wo)
            weight = F(1.0) if rd.only_direct else F(light_pdf / F(light_pdf + bounce_pdf))
            o = (t3.f3(v.point) + t3.f3(n) * F(t3.NORMAL_OFFSET * t3.signum(wo[2]))).astype(np.float32)
            sh = P.hit(o, direction)
            if sh is None or t3.tag(sh["material"]) != t3.TAG_LIGHT:
                continue
            lwi = t3.Frame(sh["normal"]).to_local(-direction)
            le = P.emission(sh["material"], lam, lwi)
            cos_i, cos_o = F(abs(lwi[2])), F(abs(wo[2]))
            c = F(F(F(F(F(F(refl * v.throughput) * cos_i) * cos_o) * le) * weight) / light_pdf)
            terminal = "%d" % groups[int(sh["instance"])]
        if c == 0:
            continue
        full = path + "DRT"[tpp.third_event(P, v, direction)] + terminal
        for e, rx in enumerate(regexes):
            if rx.fullmatch(full):
                sums[e] = F(sums.get(e, F(0.0)) + c)
    for e, s in sums.items():
        energy[e] = F(energy[e] + F(s / F(rd.light_samples)))


def third_color(P, lights, groups, regexes, pixel, sample):
    """t3.color with every contribution's path written out: K energies, one per expression."""
    rd = P.rd
    o, d0, lam = P.sc.camera_samples(rd, [pixel], [sample])
    o, d0, lam = t3.f3(o[0]), t3.f3(d0[0]), F(lam[0])
    walk = [t3.Vertex("camera", t3.f3([0, 0, 0]), o, d0, 0, 0, F(1.0), F(100.0))]
    t3.random_walk(P, o, d0, lam, pixel, sample, walk)
    energy = [F(0.0)] * len(regexes)
    path = "C"

    def add(full, value):
        for e, rx in enumerate(regexes):
            if rx.fullmatch(full):
                energy[e] = F(energy[e] + value)
    for index in range(1, len(walk)):
        prev, v = walk[index - 1], walk[index]
        if v.kind == "env":
            wo = v.normal
            cos_i = F(abs(t3.dot(prev.normal, wo)))
            with np.errstate(divide="ignore", invalid="ignore"):
                w = t3.power_heuristic(F(prev.pdf_forward / cos_i), F(t3.ENV_PDF / cos_i))
            add(path + "e", F(F(w * v.throughput) * P.env_emission(lam)))
        elif v.kind == "light":
            em = P.emission(v.material, lam, v.local_wi)
            if em > 0:
                terminal = "%d" % groups[v.instance]
                if rd.light_samples == 0 or prev.kind == "camera":
                    add(path + terminal, F(v.throughput * em))
                elif not rd.only_direct:
                    nd = t3.normalized((v.point - prev.point).astype(np.float32))
                    hyp = t3.rect_psa_pdf(dict(lights)[v.instance], t3.dot(prev.normal, nd), t3.dot(v.normal, nd), prev.point, v.point)
                    w = t3.power_heuristic(prev.pdf_forward, hyp)
                    add(path + terminal, F(F(w * v.throughput) * em))
        else:
            n = t3.normalized(v.normal)
            frame = t3.Frame(n)
            wi = frame.to_local(t3.normalized((prev.point - v.point).astype(np.float32)))
            if rd.light_samples > 0:
                third_light_samples(P, lights, groups, lam, v, n, frame, wi, pixel, sample, index - 1, path, regexes, energy)
        if index + 1 < len(walk):   # the walk continues from v: a scattering event, whose kind is that of the direction to the next vertex
            nxt = walk[index + 1]
            out_dir = nxt.normal if nxt.kind == "env" else t3.normalized((nxt.point - v.point).astype(np.float32))
            path += "DRT"[tpp.third_event(P, v, out_dir)]
    xyz = P.xyz_bar(lam)
    return [(xyz * e).astype(np.float32) for e in energy]


def third_render(P, lights, groups, regexes):
    rd, K = P.rd, len(regexes)
    films = np.zeros((K, rd.height, rd.width, 4), np.float32)
    for y in range(rd.height):
        for x in range(rd.width):
            px, temp = np.zeros((K, 3), np.float32), np.zeros((K, 3), np.float32)
            for s in range(rd.spp):
                temp = (temp + np.stack(third_color(P, lights, groups, regexes, y * rd.width + x, s))).astype(np.float32)
                if (s + 1) % 10 == 0 or s + 1 == rd.spp:
                    px = (px + temp).astype(np.float32)
                    temp = np.zeros((K, 3), np.float32)
            films[:, y, x, :3] = px / F(rd.spp)
    return films


THIRD = ("CD[RT]+[LE]", "C.*T.*L2", "CT+(D|R)?[L1E1]")   # caustics; the second lamp's light that crossed glass; group-labelled terminals behind the pane


@pytest.mark.parametrize("kw", [{}, {"light_samples": 3}], ids=["L2", "L3"])
def test_expressions_agree_with_a_third_reading(pkg, oracle, emu_px, kw):
    """The films of a caustic expression and of two group-labelled ones, from the scalar-Python walk that writes out each contribution's path and applies `re`,
    agree with the emulation's under the third reading's own bar, max |d| / max(|ref|, 1e-3) < 2e-5, every pixel, channel and expression."""
    b = lamps_behind_a_pane(pkg)
    lights = [(i, t3.rect_of(b, i)) for i, inst in enumerate(b.instances) if inst.kind == pkg.api.SHAPE_RECT and t3.tag(inst.material) == t3.TAG_LIGHT]
    assert [i for i, _ in lights] == [0, 4]
    groups, env_group = (1, 0, 0, 0, 2, 0), 1
    rd = pkg.api.render_desc(16, 12, 3, 6, **kw)
    mine = third_render(t3.Probes(pkg, oracle, b, rd), lights, groups, [to_re(e, env_group) for e in THIRD])
    film, ref, _ = emu_px.create_scene(b).render_path_exprs(rd, THIRD, groups, env_group)
    assert np.isfinite(mine).all() and np.isfinite(ref).all()
    rel = np.abs(mine - ref)[..., :3] / np.maximum(np.abs(ref[..., :3]), 1e-3)
    for k, expr in enumerate(THIRD):
        print("%-18s worst %.3g  lit %d" % (expr, float(rel[k].max()), int((ref[k][..., :3] != 0).any(axis=-1).sum())))
    assert all(ref[k].any() for k in range(len(THIRD)))
    assert rel.max() < 2e-5, float(rel.max())


# ---- the surface
def test_refusals(pkg, emu_px):
    """Every refusal returns its status and a message of its own; the product runs the same checks before it looks for a device."""
    a = pkg.api
    sc = emu_px.create_scene(pkg.scene.light_groups_room())
    ok = dict(width=8, height=8, spp=10, max_bounces=3)
    cases = [
        ("hero", a.render_desc(hero_wavelengths=4, **ok), a.PT_ERR_UNSUPPORTED, "one wavelength"),
        ("medium", a.render_desc(medium_aware=True, **ok), a.PT_ERR_UNSUPPORTED, "medium-aware"),
        ("shard", a.render_desc(shard=(0, 2), **ok), a.PT_ERR_UNSUPPORTED, "whole film"),
        ("range", a.render_desc(first_sample=0, sample_count=5, **ok), a.PT_ERR_UNSUPPORTED, "whole sample range"),
    ]
    seen = set()
    for name, rd, status, word in cases:
        with pytest.raises(a.PtError) as e:
            sc.render_path_exprs(rd, "CL")
        assert e.value.status == status and word in str(e.value) and "path expressions" in str(e.value), (name, str(e.value))
        seen.add(str(e.value))
    assert len(seen) == 4
    rd = a.render_desc(**ok)
    good = emu_px.path_expr_compile(["CD+L", "CE"])

    def broken(**fields):
        p = a.PathExprProgram.from_buffer_copy(good)
        for k, v in fields.items():
            setattr(p, k, v)
        return p
    successor, mask, stray = broken(), broken(), broken()
    successor.table[0][0] = good.table[0][0] | 63 << 6          # a successor behind R that is no state
    mask.table[good.start][1] |= 4                               # bit 2 of a program with two outputs
    stray.table[0][3] |= 1 << 8                                  # beyond the ninth mask
    for p, word in ((broken(outputs=0), "outputs must be in 1..8"), (broken(outputs=9), "outputs must be in 1..8"), (broken(states=0), "states must be in 1..64"),
                    (broken(states=65), "states must be in 1..64"), (broken(start=good.states), "start"), (broken(environment_group=8), "environment_group"),
                    (successor, "successor"), (mask, "masks of its outputs"), (stray, "masks of its outputs")):
        with pytest.raises(a.PtError) as e:
            sc.render_path_exprs(rd, p)
        assert e.value.status == a.PT_ERR_INVALID_ARGUMENT and word in str(e.value) and "path expression program" in str(e.value), str(e.value)
    for ids, word in (((0, 0, 1), "the scene has 6 instances"), ((0, 0, 8, 0, 0, 0), "instance 2 is in group 8")):
        with pytest.raises(a.PtError) as e:
            sc.render_path_exprs(rd, good, ids)
        assert e.value.status == a.PT_ERR_INVALID_ARGUMENT and word in str(e.value), str(e.value)
    fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    film = np.zeros((8, 8, 4), f32).ctypes.data_as(fp)
    emu_px.lib.ptemu_light_groups_last_error.restype = C.c_char_p
    entry, error = emu_px._render_path_exprs, lambda: emu_px.lib.ptemu_light_groups_last_error().decode()
    assert entry(None, C.byref(rd), C.byref(good), None, 0, film, None, None) == 1 and error() == "the scene is null"
    assert entry(sc.handle, None, C.byref(good), None, 0, film, None, None) == 1 and error() == "the render desc is null"
    assert entry(sc.handle, C.byref(rd), None, None, 0, film, None, None) == 1 and error() == "the path expression program is null"
    assert entry(sc.handle, C.byref(rd), C.byref(good), None, 0, None, None, None) == 1 and error() == "film_xyzw is null"
    assert entry(sc.handle, C.byref(rd), C.byref(good), None, 6, film, None, None) == 1 and "n_instances must be 0" in error()
    # the product runs the same checks before it looks for a device: without a scene the first of them is the one that can be seen — of both entries
    L = pkg.load()
    assert L._render_path_exprs(None, C.byref(rd), C.byref(good), None, 0, film, None, None) == 1 and L.last_error() == "the scene is null"
    ad = a.AdaptiveDesc(40, 10, 0.1, 0.0)
    counts = np.zeros((8, 8), np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
    assert L._render_adaptive_path_exprs(None, C.byref(rd), C.byref(ad), C.byref(good), None, 0, film, counts, None, None, None) == 1 and L.last_error() == "the scene is null"


def test_header_constants_and_binding_rows(pkg, tmp_path):
    """The header's constants are the Python mirror's, the program has the compiler's size and offsets, the four entries are exported and bound."""
    a = pkg.api
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_light_groups_denoise.h"\nint main(void) { printf("%d %d %d %d %zu %zu %zu %zu", PT_PATH_EXPRS_MAX, '
                   'PT_PATH_EXPR_STATES_MAX, PT_PATH_EXPR_TERMINALS, PT_PATH_EXPR_ENVIRONMENT, sizeof(pt_path_expr_program), offsetof(pt_path_expr_program, start), '
                   'offsetof(pt_path_expr_program, environment_group), offsetof(pt_path_expr_program, table)); return 0; }\n')
    exe = tmp_path / "consts"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = a.PathExprProgram
    assert got == [a.PATH_EXPRS_MAX, a.PATH_EXPR_STATES_MAX, a.PATH_EXPR_TERMINALS, a.PATH_EXPR_ENVIRONMENT, C.sizeof(P), P.start.offset, P.environment_group.offset, P.table.offset]
    assert got[:5] == [8, 64, 9, 8, 16 + 64 * 16]
    lib = C.CDLL(pkg.load().path)
    rows = (("path_expr_compile", "pt_light_groups.h", 6), ("path_expr_match", "pt_light_groups.h", 3), ("render_path_exprs", "pt_light_groups.h", 8),
            ("render_adaptive_path_exprs", "pt_light_groups_denoise.h", 11))
    for name, header, n_args in rows:
        assert getattr(lib, "pt_" + name) is not None
        assert name in a.ENTRIES and name in [e.name for h, rows_ in a.BINDINGS if h == header for e in rows_]
        assert ("pt_" + name + "(") in open(os.path.join(ROOT, "include", header)).read()
        assert len(a.ENTRIES[name].argtypes) == n_args
    rules = open(os.path.join(CSRC, "pt_path_expr_rules.h")).read()
    assert "PX_MAX_EXPRS = 8" in rules and "PX_MAX_STATES = 64" in rules and "PX_ENVIRONMENT = 8" in rules


def test_sanitizer_program(tmp_path):
    """tools/path_exprs_sanitize.cpp, a stand-alone host binary built with the address and undefined-behaviour sanitizers: the compiler, the match and the
    router's rules over a poisoned state plane in a heap buffer of exactly the engine's size."""
    exe = str(tmp_path / "path_exprs_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wno-unknown-pragmas",
                           "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tools", "path_exprs_sanitize.cpp"), os.path.join(CSRC, "pt_path_expr.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stderr[-2000:]


PTCLI_EXPRS = "caustics=CD[RT]+[LE];all = C.*[LE] ;direct=C.?L0"
PTCLI_NAMES = ("caustics", "all", "direct")


def test_ptcli_flag_refusals(pkg):
    """--path-exprs is refused with the flags --path-passes is refused with, and with --path-passes itself; a bad list or expression exits with status 2 and the
    compiler's own message before any file is read; the help and the file's head name the flags."""
    exe = ptcli(pkg)
    px = ["--path-exprs", "a=CL"]
    cases = [(px + extra, "--path-exprs cannot be combined with " + extra[0]) for extra in (
        ["--adaptive", "0.1"], ["--spectral-bins", "8"], ["--denoise-spectral-bins", "8"], ["--devices", "1"], ["--spectral-devices", "1"],
        ["--hero-wavelengths", "4"], ["--light-groups", "instance"], ["--denoise-light-groups", "instance"], ["--relamp-groups", "instance"], ["--light-group-devices", "1"],
        ["--path-passes"], ["--denoise"])]
    cases += [
        (["--path-expr-groups", "instance"], "--path-expr-groups needs --path-exprs"),
        (px + ["--path-expr-groups", "colour"], "--path-expr-groups needs `instance` or `material`"),
        (["--path-exprs", "CL"], "--path-exprs takes NAME=EXPR;NAME=EXPR"),
        (["--path-exprs", "a=CL;a=CE"], "--path-exprs names 'a' twice"),
        (["--path-exprs", "a/b=CL"], "--path-exprs: the name 'a/b'"),
        (["--path-exprs", ";".join("n%d=CL" % i for i in range(9))], "--path-exprs takes at most 8 expressions"),
        (["--path-exprs", "a=CL;b=CD(L"], "--path-exprs: expression 1, column 4: "),
    ]
    for args, message in cases:
        r = subprocess.run([exe, "--config", "/nonexistent/config.toml"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and ("error: " + message) in r.stderr, (args, r.stderr)
    assert "[--path-exprs NAME=EXPR;...] [--path-expr-groups instance|material]" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr
    assert "[--path-exprs NAME=EXPR;...] [--path-expr-groups instance|material]" in open(os.path.join(CSRC, "host", "ptcli.cpp")).read().split("#include")[0]


def test_ptcli_dry_run(pkg, tmp_path):
    """A dry run with the flag loads the scene, names the expressions and the program's size and ends well."""
    cfg = tmp_path / "config.toml"
    cfg.write_text(tpp.scaled_c2_config(pkg))
    base = [ptcli(pkg), "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / "out"), "-n"]
    for extra in ([], ["--path-expr-groups", "material"]):
        ok = subprocess.run(base + ["--path-exprs", PTCLI_EXPRS] + extra, capture_output=True, text=True, cwd=str(tmp_path))
        assert ok.returncode == 0 and re.search(r"path expressions: 3 \(caustics, all, direct\), \d+ states", ok.stdout), (ok.stdout, ok.stderr)


# ------------------------------------------------------------------------------------------------ GPU tier
def pane_scene(engine, pkg, batch_slots=0, flags=0):
    return engine.create_scene(pkg.scene.path_passes_room(), tuning=tpp.clean_tuning(engine, pkg, batch_slots, flags))


@pytest.fixture(scope="module")
def pane_gpu(engine, pkg):
    """The engine's renders of the room behind the pane on one scene handle, made once: pt_render, the five overlapping expressions at light_samples 2 and 3."""
    sc = pane_scene(engine, pkg)
    out = {"scene": sc, "plain": sc.render(pane_rd(pkg))}
    for L in (2, 3):
        film, films, prof = sc.render_path_exprs(pane_rd(pkg, L), OVERLAP, PANE_GROUPS, PANE_ENV_GROUP)
        out[L] = {"film": film, "films": films, "prof": prof}
    out["resident"] = sc.light_groups_resident()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2, 3])
def test_gpu_engine_is_the_emulation(pane_gpu, pane_emu, L):
    """Film, the five expression films and the counters are the emulation's bit for bit; at light_samples 2 the film is pt_render's on the same handle."""
    g, e = pane_gpu[L], pane_emu[L]
    assert same_bits(g["film"], e["film"]) and counters(g["prof"]) == counters(e["prof"])
    for k, expr in enumerate(OVERLAP):
        assert same_bits(g["films"][k], e["films"][k]), expr
    if L == 2:
        assert same_bits(g["film"], pane_gpu["plain"][0]) and counters(g["prof"]) == counters(pane_gpu["plain"][1])
    assert pane_gpu["resident"] == (24, 16, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["overlap", "no_overlap", "no_lds"])
def test_gpu_passes_and_tunings_keep_the_bits(engine, pkg, pane_gpu, variant):
    """pt_tuning::batch_slots 1024, the smallest the engine takes, cuts the 24 x 16 x 8 = 3072 slots into three passes, so the first set of pass buffers — with a
    state plane of its own, as the second has — is used twice and the third pass finds the first one's state words there; with the pass overlap, without it, and
    without LDS staging."""
    flags = {"overlap": 0, "no_overlap": pkg.api.TUNE_NO_PASS_OVERLAP, "no_lds": pkg.api.TUNE_NO_LDS}[variant]
    sc = pane_scene(engine, pkg, 1024, flags)
    film, films, prof = sc.render_path_exprs(pane_rd(pkg, 3), OVERLAP, PANE_GROUPS, PANE_ENV_GROUP)
    print("passes:", prof.kernel_launches[0])
    assert prof.kernel_launches[0] == 3
    g = pane_gpu[3]
    assert same_bits(film, g["film"]) and same_bits(films, g["films"]) and counters(prof) == counters(g["prof"])


@pytest.mark.gpu
def test_gpu_nine_passes_keep_the_bits(engine, pkg, emu_px):
    """Cut into nine passes.  A pass holds at least 1024 slots (the engine's floor for batch_slots), so 8 spp on 24 x 16 pixels make three passes at the most; the
    same film at 24 spp — two phases of ten and a remainder — with batch_slots 1280 makes nine: three chunks of 128 pixels, each continued over the samples
    0..10, 10..20 and 20..24.  Against the emulation at that count, bit for bit."""
    rd = pkg.api.render_desc(24, 16, 24, 5, light_samples=3, seed=7)
    film, films, prof = pane_scene(engine, pkg, 1280).render_path_exprs(rd, OVERLAP, PANE_GROUPS, PANE_ENV_GROUP)
    assert prof.kernel_launches[0] == 9
    wfilm, wfilms, wprof = emu_px.create_scene(pkg.scene.path_passes_room()).render_path_exprs(rd, OVERLAP, PANE_GROUPS, PANE_ENV_GROUP)
    assert same_bits(film, wfilm) and same_bits(films, wfilms) and counters(prof) == counters(wprof)


@pytest.mark.gpu
def test_gpu_identities_with_path_passes_and_light_groups(engine, pkg):
    """On the engine itself: the built-in expressions against pt_render_path_passes on the room behind the pane, C.*[LgEg] against pt_render_light_groups on the
    room, per plane with numpy.array_equal."""
    rd = tpp.room_rd(pkg)
    sc = pane_scene(engine, pkg)
    wfilm, passes, wprof = sc.render_path_passes(rd)
    film, films, prof = sc.render_path_exprs(rd, pkg.api.PATH_PASS_EXPRS)
    assert same_bits(film, wfilm) and counters(prof) == counters(wprof) and sc.light_groups_resident() == (24, 24, 8)
    planes_equal(films, passes, tpp.NAMES)
    assert all(passes[c][..., :3].any() for c in range(8))
    room = engine.create_scene(pkg.scene.light_groups_room(), tuning=tpp.clean_tuning(engine, pkg))
    wfilm, groups, wprof = room.render_light_groups(rd, ROOM_GROUPS, ROOM_ENV_GROUP)
    film, films, prof = room.render_path_exprs(rd, group_exprs(3), ROOM_GROUPS, ROOM_ENV_GROUP)
    assert same_bits(film, wfilm) and counters(prof) == counters(wprof) and room.light_groups_resident() == (24, 24, 3)
    planes_equal(films, groups, ("rect lamp", "disk lamp", "sky"))


AD = tpp.AD   # tests/test_light_groups_denoise.py's adaptive case


@pytest.fixture(scope="module")
def adaptive_gpu(engine, pkg):
    rd = tpp.adaptive_rd(pkg)
    sc = pane_scene(engine, pkg)
    plain = sc.render_adaptive(rd, AD["max_samples"], AD["rel_error"], step=AD["step"], stats=True)
    film, counts, stats, films, prof = sc.render_adaptive_path_exprs(rd, AD["max_samples"], AD["rel_error"], OVERLAP, PANE_GROUPS, PANE_ENV_GROUP, step=AD["step"], stats=True)
    return {"rd": rd, "scene": sc, "plain": plain, "film": film, "counts": counts, "stats": stats, "films": films, "prof": prof}


@pytest.mark.gpu
def test_gpu_adaptive_entry(engine, pkg, adaptive_gpu):
    """Film, counts and statistics are pt_render_adaptive's bit for bit; each pixel's expression films are pt_render_path_exprs' at that pixel's own count."""
    g = adaptive_gpu
    film, counts, stats, prof = g["plain"]
    values, n = np.unique(g["counts"], return_counts=True)
    print("counts:", dict(zip(values.tolist(), n.tolist())))
    assert len(values) >= 2
    assert same_bits(g["film"], film) and np.array_equal(g["counts"], counts) and np.array_equal(g["stats"].view(np.uint64), stats.view(np.uint64))
    assert counters(g["prof"]) == counters(prof) and g["prof"].kernel_launches[5] == prof.kernel_launches[5]
    other = pane_scene(engine, pkg)
    for v in values:
        ffilm, ffilms, _ = other.render_path_exprs(tpp.adaptive_rd(pkg, int(v)), OVERLAP, PANE_GROUPS, PANE_ENV_GROUP)
        at = g["counts"] == v
        assert same_bits(g["film"][at], ffilm[at]), v
        for k, expr in enumerate(OVERLAP):
            assert same_bits(g["films"][k][at], ffilms[k][at]), (v, expr)
    assert not g["films"][..., 3].any() and np.isfinite(g["films"]).all()


@pytest.mark.gpu
def test_gpu_resident_mix_and_filter_follow_an_expression_render(engine, pkg, adaptive_gpu):
    """The expression films are the scene's resident group films: the resident mix is pt_light_groups_mix of the films read back, and after the adaptive entry
    pt_denoise_light_groups_resident equals pt_denoise_light_groups over the host arrays, bit for bit."""
    g = adaptive_gpu
    sc, rd = g["scene"], g["rd"]
    assert sc.light_groups_resident() == (24, 24, 5) and sc.resident_info()[3] & pkg.api.RESIDENT_FILM
    rng = np.random.default_rng(5)
    m = (rng.random((5, 3, 3), dtype=f32) * f32(2.0) - f32(0.5)).astype(f32)
    assert same_bits(sc.light_groups_mix_resident(m), engine.light_groups_mix(g["films"], m)) and same_bits(sc.light_groups_mix_resident(m), tpp.mix_numpy(g["films"], m))
    sc.resident_guides(rd, 4)
    host_guides = pane_scene(engine, pkg).render_guides(rd, 4)
    den, var, den_films = sc.denoise_light_groups_resident(variance=True)
    want = engine.denoise_light_groups(g["film"], g["counts"], g["stats"], host_guides, g["films"], variance=True)
    assert same_bits(den, want[0]) and same_bits(den_films, want[1]) and same_bits(var, want[2])
    assert sc.light_groups_denoised_resident() == (24, 24, 5)
    _, none, _ = sc.render_path_exprs(pane_rd(pkg), "CD[RT]+[LE]", read_films=False)
    assert none is None and sc.light_groups_resident() == (24, 16, 1)


@pytest.mark.gpu
def test_gpu_entry_refusals(engine, pkg):
    """The engine's entries refuse what the checks refuse before anything is rendered, and leave no resident films."""
    a = pkg.api
    sc = engine.create_scene(pkg.scene.light_groups_room())
    ok = dict(width=8, height=8, spp=10, max_bounces=3)
    bad = engine.path_expr_compile("CL")
    bad.table[0][0] = 63
    for call, status, word in ((lambda: sc.render_path_exprs(a.render_desc(hero_wavelengths=4, **ok), "CL"), a.PT_ERR_UNSUPPORTED, "path expressions carry one wavelength"),
                               (lambda: sc.render_path_exprs(a.render_desc(**ok), bad), a.PT_ERR_INVALID_ARGUMENT, "successor"),
                               (lambda: sc.render_path_exprs(a.render_desc(**ok), "CL", (0, 1)), a.PT_ERR_INVALID_ARGUMENT, "the scene has 6 instances"),
                               (lambda: sc.render_adaptive_path_exprs(a.render_desc(shard=(0, 2), **ok), 40, 0.1, "CL"), a.PT_ERR_UNSUPPORTED, "whole film"),
                               (lambda: sc.render_adaptive_path_exprs(a.render_desc(**ok), 5, 0.1, "CL"), a.PT_ERR_INVALID_ARGUMENT, "max_samples")):
        with pytest.raises(a.PtError) as e:
            call()
        assert e.value.status == status and word in str(e.value), str(e.value)
    assert sc.light_groups_resident() is None


@pytest.mark.gpu
def test_gpu_ptcli_path_exprs(pkg, tmp_path):
    """ptcli --path-exprs on the Cornell config writes one file per expression; the usual outputs are byte for byte those of a run without the flag, and the
    "all" expression's file is the film's."""
    cfg = tmp_path / "config.toml"
    cfg.write_text(tpp.scaled_c2_config(pkg))
    base = [ptcli(pkg), "--root", pkg.PACKAGE_DIR, "--config", str(cfg)]

    def run(out, *extra):
        return subprocess.run(base + ["--output-dir", str(tmp_path / out)] + list(extra), capture_output=True, text=True, cwd=str(tmp_path), timeout=120)

    def data(d, f):
        return open(tmp_path / d / f, "rb").read()
    plain, split = run("plain"), run("split", "--path-exprs", PTCLI_EXPRS, "--path-expr-groups", "instance")
    assert plain.returncode == 0 and split.returncode == 0, (plain.stderr, split.stderr)
    usual = sorted(os.listdir(tmp_path / "plain"))
    assert usual and all(data("plain", f) == data("split", f) for f in usual)
    extra = sorted(set(os.listdir(tmp_path / "split")) - set(usual))
    stem = usual[0].rsplit(".", 1)[0]
    assert extra == sorted("%s_expr_%s.exr" % (stem, n) for n in PTCLI_NAMES), extra
    assert len({data("split", f) for f in extra}) == 3   # (no caustics in a Lambertian box, everything, the lamp seen or sampled from the first vertex)
    assert data("split", "%s_expr_all.exr" % stem) == data("plain", "%s.exr" % stem)
