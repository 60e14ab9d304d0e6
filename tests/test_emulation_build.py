"""The emulation builder (tests/emulation.py) on a toy tree: a.cpp includes h.h, which includes g.h; b.cpp includes neither; library `one` is a + b, library `two`
is b alone.  What is rebuilt, and what is not, is read from mtimes and inodes; time moves by os.utime, never by waiting."""
import ctypes as C
import itertools
import os
import shutil

import pytest

import emulation

TABLE = {"one": "a.cpp b.cpp", "two": "b.cpp"}
FLAGS = ("-O1", "-fPIC")


@pytest.fixture()
def toy(tmp_path):
    src = tmp_path / "src"
    src.mkdir()
    (src / "g.h").write_text("#define G 40\n")
    (src / "h.h").write_text('#include "g.h"\n#define H (G + 2)\n')
    (src / "a.cpp").write_text('#include "h.h"\nextern "C" int ptemu_a() { return H; }\n')
    (src / "b.cpp").write_text('extern "C" int ptemu_b() { return 7; }\n')
    build = tmp_path / "out" / "build"

    def make(name, flags=FLAGS):
        return emulation.library_path(name, table=TABLE, roots=(str(src),), build_dir=str(build), flags=flags)
    return src, build, make


_COPIES = itertools.count()


def load(path):
    """The library as it stands now: dlopen answers a path it has seen with the library it loaded then, so each load goes through a copy under a fresh name."""
    copy = "%s.%d" % (path, next(_COPIES))
    shutil.copy(path, copy)
    return C.CDLL(copy)


def stamps(build):
    """(mtime, inode) of every object and library of the toy tree"""
    paths = [build / "a.o", build / "b.o", build.parent / "libptemu_one.so", build.parent / "libptemu_two.so"]
    return {p.name: (os.stat(p).st_mtime_ns, os.stat(p).st_ino) for p in paths}


def changed(before, after):
    return {k for k in before if before[k] != after[k]}


def forward(path, seconds=10):
    """`path` modified `seconds` after the newest file the toy tree has so far"""
    newest = max(os.stat(os.path.join(d, f)).st_mtime_ns for d, _, files in os.walk(path.parent.parent) for f in files)
    os.utime(path, ns=(newest + seconds * 10**9,) * 2)


def test_first_build_loads_and_second_call_writes_nothing(toy):
    src, build, make = toy
    one, two = load(make("one")), load(make("two"))
    assert (one.ptemu_a(), one.ptemu_b(), two.ptemu_b()) == (42, 7, 7)
    assert not hasattr(two, "ptemu_a")
    assert os.path.basename(make("one")) == "libptemu_one.so" and os.path.dirname(make("one")) == str(build.parent)
    before = stamps(build)
    make("one"), make("two")
    assert changed(before, stamps(build)) == set()
    assert not [f for d in (build, build.parent) for f in os.listdir(d) if ".tmp" in f]   # nothing half-written is left


def test_nested_header_rebuilds_what_reads_it_and_nothing_else(toy):
    src, build, make = toy
    make("one"), make("two")
    before = stamps(build)
    (src / "g.h").write_text("#define G 50\n")
    forward(src / "g.h")
    make("one"), make("two")
    assert changed(before, stamps(build)) == {"a.o", "libptemu_one.so"}
    assert load(make("one")).ptemu_a() == 52


def test_changed_flags_rebuild_every_object(toy):
    src, build, make = toy
    make("one"), make("two")
    before = stamps(build)
    make("one", FLAGS + ("-DUNUSED=1",)), make("two", FLAGS + ("-DUNUSED=1",))
    assert changed(before, stamps(build)) == {"a.o", "b.o", "libptemu_one.so", "libptemu_two.so"}
    before = stamps(build)
    make("one", FLAGS + ("-DUNUSED=1",)), make("two", FLAGS + ("-DUNUSED=1",))
    assert changed(before, stamps(build)) == set()


@pytest.mark.parametrize("how", ["no record", "a library another recipe wrote"])
def test_library_without_its_record_is_relinked(toy, how):
    src, build, make = toy
    make("one"), make("two")
    lib = build.parent / "libptemu_two.so"
    if how == "no record":
        os.remove(build / "libptemu_two.so.objects")
    else:
        lib.write_bytes(b"not a library")
        forward(lib)
    before = stamps(build)
    assert load(make("two")).ptemu_b() == 7
    assert changed(before, stamps(build)) == {"libptemu_two.so"}
    before = stamps(build)
    make("two")
    assert changed(before, stamps(build)) == set()


def test_deleted_header_named_in_a_depfile(toy):
    src, build, make = toy
    make("one"), make("two")
    assert str(src / "g.h") in (build / "a.d").read_text()
    (src / "h.h").write_text("#define H 9\n")   # the include of g.h is gone, and so is g.h
    os.remove(src / "g.h")
    forward(src / "h.h")
    before = stamps(build)
    assert load(make("one")).ptemu_a() == 9
    make("two")
    assert changed(before, stamps(build)) == {"a.o", "libptemu_one.so"}
    assert "g.h" not in (build / "a.d").read_text()
    # and with nothing but the deletion: the source no longer reads h.h, the depfile still names it
    (src / "a.cpp").write_text('extern "C" int ptemu_a() { return 3; }\n')
    os.utime(src / "a.cpp", ns=(os.stat(build / "a.o").st_mtime_ns - 10**9,) * 2)   # older than its object: only the missing header says "stale"
    os.remove(src / "h.h")
    assert load(make("one")).ptemu_a() == 3
