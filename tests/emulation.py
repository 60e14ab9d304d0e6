"""The one place that knows how a host emulation library is made.  TABLE names each library's sources; every source is compiled once to an object under
host_emulation/build/ and the libraries are linked from the objects.  What an object depends on is the compiler's to say (-MMD), so a new feature adds a row
here, never a header list.  Every file is written under a temporary name and renamed, so two processes building at once never load half a library."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "host_emulation")
CSRC = os.path.join(ROOT, "rust-pathtracer_amd", "csrc")
ROOTS = (EMU_DIR, CSRC, os.path.join(ROOT, "tools"))   # where a row's file names are looked up, in this order
BUILD_DIR = os.path.join(EMU_DIR, "build")             # objects, depfiles and records; the libraries go beside it
# -ffp-contract=off -fno-fast-math: the numeric contract of include/pt_numerics.h
FLAGS = ("-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-value")

HOST = " pt_scene_host.cpp pt_plan.cpp"   # the engine's own host sources
DENOISE = "ptemu.cpp ptemu_adaptive.cpp ptemu_denoise.cpp"
ALBEDO = DENOISE + " ptemu_denoise_albedo.cpp"
CHAIN = ALBEDO + " ptemu_guides_chain.cpp"
JOINT = CHAIN + " ptemu_denoise_spectral.cpp ptemu_denoise_spectral_albedo.cpp"
# library name -> sources; the file is libptemu_<name>.so, or lib<name>.so for a name that begins with "pt"
TABLE = {
    "ptemu": "ptemu.cpp" + HOST,
    "adaptive": "ptemu.cpp ptemu_adaptive.cpp" + HOST,
    "adaptive_multi": "ptemu.cpp ptemu_adaptive.cpp ptemu_adaptive_multi.cpp" + HOST,
    "denoise": DENOISE + HOST,
    "denoise_albedo": ALBEDO + HOST,
    "guides_chain": CHAIN + HOST,
    "denoise_spectral": DENOISE + " ptemu_denoise_spectral.cpp" + HOST,
    "denoise_spectral_albedo": JOINT + HOST,
    "denoise_resident": JOINT + " ptemu_spectral_project.cpp ptemu_denoise_resident.cpp" + HOST,
    "spectral": "ptemu_spectral.cpp pt_plan.cpp",
    "spectral_project": "ptemu_spectral_project.cpp pt_plan.cpp pt_scene_host.cpp",
    "spectral_shard": "ptemu_spectral_shard.cpp pt_plan.cpp",
    "resident_assemble": "ptemu_resident_assemble.cpp ptemu_spectral_shard.cpp pt_plan.cpp",
    "light_groups_shard": "ptemu_light_groups_shard.cpp pt_plan.cpp",
    "light_groups": "ptemu.cpp ptemu_light_groups.cpp" + HOST,
    "light_groups_spectral": "ptemu.cpp ptemu_light_groups.cpp ptemu_spectral_project.cpp ptemu_light_groups_spectral.cpp" + HOST,
    "light_groups_denoise": "ptemu.cpp ptemu_adaptive.cpp ptemu_light_groups.cpp ptemu_adaptive_light_groups.cpp ptemu_denoise.cpp ptemu_denoise_albedo.cpp "
                            "ptemu_guides_chain.cpp ptemu_denoise_spectral.cpp ptemu_denoise_spectral_albedo.cpp ptemu_denoise_light_groups.cpp" + HOST,
    "path_passes": "ptemu.cpp ptemu_path_passes.cpp" + HOST,
    "matte": "ptemu.cpp ptemu_matte.cpp" + HOST,
    "mesh_lights": "ptemu.cpp ptemu_light.cpp" + HOST,
    # the experiments under tools/: each .cpp includes ptemu.cpp with its own recording switched on
    "ptlightwalks": "light_walks.cpp" + HOST,
    "ptcandstats": "candidate_stats.cpp" + HOST,
    "ptliverays": "live_rays.cpp" + HOST,
    "ptwalkstats": "walk_stats.cpp" + HOST,
}


def _read(path):
    try:
        with open(path) as f:
            return f.read()
    except OSError:
        return None


def _write(path, text):
    tmp = "%s.%d.tmp" % (path, os.getpid())
    with open(tmp, "w") as f:
        f.write(text)
    os.replace(tmp, path)


def _newer(paths, than):
    """Is one of `paths` gone, or modified after the file `than`?"""
    t = os.stat(than).st_mtime_ns
    return any(not os.path.exists(p) or os.stat(p).st_mtime_ns > t for p in paths)


def _object(src, build_dir, flags):
    """The object of `src`, compiled if it, its depfile or its flag record is missing, the flags differ, or a file its depfile names is newer or gone."""
    stem = os.path.join(build_dir, os.path.splitext(os.path.basename(src))[0])
    obj, dep, rec = stem + ".o", stem + ".d", stem + ".flags"
    made = _read(dep)
    stale = not os.path.exists(obj) or made is None or _read(rec) != " ".join(flags)
    if not stale:   # the depfile's first rule, "<object>: <source> <header> ..." over continued lines; after it one empty rule per header (-MP)
        stale = _newer(made.replace("\\\n", " ").split("\n", 1)[0].split(":", 1)[1].split(), obj)
    if stale:
        tmp = "%s.%d.tmp" % (stem, os.getpid())
        subprocess.check_call(["g++", *flags, "-MMD", "-MP", "-MF", tmp + ".d", "-c", "-o", tmp + ".o", src])
        os.replace(tmp + ".d", dep)
        os.replace(tmp + ".o", obj)
        _write(rec, " ".join(flags))
    return obj


def library_path(name, table=TABLE, roots=ROOTS, build_dir=BUILD_DIR, flags=FLAGS):
    """The path of library `name`, its objects compiled and the library linked first where they are stale.  A library is stale if it is missing, if an object is
    newer, or if the record of its last link (the object list and the library's own mtime) is not what stands there: no record, or a file that some other
    recipe wrote."""
    os.makedirs(build_dir, exist_ok=True)
    srcs = [next(p for p in (os.path.join(r, f) for r in roots) if os.path.exists(p)) for f in table[name].split()]
    objs = [_object(s, build_dir, flags) for s in srcs]
    lib = os.path.join(os.path.dirname(build_dir), "lib%s.so" % (name if name.startswith("pt") else "ptemu_" + name))
    rec = os.path.join(build_dir, os.path.basename(lib) + ".objects")

    def record():
        return "\n".join(objs + [str(os.stat(lib).st_mtime_ns)])
    if not os.path.exists(lib) or _read(rec) != record() or _newer(objs, lib):
        tmp = "%s.%d.tmp" % (lib, os.getpid())
        subprocess.check_call(["g++", "-shared", "-o", tmp] + objs)
        os.replace(tmp, lib)
        _write(rec, record())
    return lib


def load(pkg, name):
    return pkg.api.Library(library_path(name), "ptemu_", optional=("render_device", "device_info"))
