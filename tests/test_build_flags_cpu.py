"""charls_amd/build.py decides object by object what to compile again.  The compiler and the linker are replaced by
recorders here (no real compile): a build with other CHARLS_AMD_CXXFLAGS, `force`, and a change to one of the two headers
the device units reach through runtime.h must each compile what they make stale."""
import os
import shutil

import pytest

from charls_amd import build as b


class _Done:
    returncode = 0

    def communicate(self):
        return b"", None


@pytest.fixture
def fake_build(monkeypatch, tmp_path):
    """build() with its outputs under tmp_path; returns (run, compiled): run(force) -> the sources compiled by that call."""
    # (a copy of the sources, so that the test that touches a header leaves the real tree's times alone)
    root = str(tmp_path / "tree")
    shutil.copytree(b.CSRC, os.path.join(root, "charls_amd", "csrc"))
    shutil.copytree(os.path.join(b.ROOT, "include"), os.path.join(root, "include"))
    monkeypatch.setattr(b, "ROOT", root)
    monkeypatch.setattr(b, "CSRC", os.path.join(root, "charls_amd", "csrc"))
    out_dir = str(tmp_path / "lib")
    monkeypatch.setattr(b, "OUT_DIR", out_dir)
    monkeypatch.setattr(b, "OUT", os.path.join(out_dir, "libcharls_amd.so"))
    monkeypatch.setattr(b, "OUT_ALIAS", os.path.join(out_dir, "libcharls.so.3"))
    monkeypatch.setenv("CHARLS_AMD_SKIP_SCRATCH_CHECK", "1")
    monkeypatch.delenv("CHARLS_AMD_CXXFLAGS", raising=False)
    compiled, flags_seen = [], []

    def start_compile(cmd):
        src, obj = cmd[cmd.index("-c") + 1], cmd[cmd.index("-o") + 1]
        compiled.append(os.path.relpath(src, b.CSRC))
        flags_seen.append([a for a in cmd if a.startswith("-D")])
        with open(obj, "w") as f:
            f.write("object")
        return _Done()

    def link(cmd):
        with open(cmd[cmd.index("-o") + 1], "w") as f:
            f.write("library")

    monkeypatch.setattr(b, "_start_compile", start_compile)
    monkeypatch.setattr(b, "_link", link)

    def run(force=False):
        del compiled[:], flags_seen[:]
        b.build(force=force)
        return sorted(compiled), list(flags_seen)

    return run


def test_plain_build_after_a_build_with_flags_compiles_every_object_again(fake_build, monkeypatch):
    first, _ = fake_build()
    assert first == sorted(b.SOURCES)
    assert fake_build()[0] == []  # nothing changed: nothing compiled
    monkeypatch.setenv("CHARLS_AMD_CXXFLAGS", "-DJLS_PHASE_CLOCKS")
    with_flags, flags = fake_build()
    assert with_flags == sorted(b.SOURCES) and all(f == ["-DJLS_PHASE_CLOCKS"] for f in flags)
    assert fake_build()[0] == []  # the same flags again: the instrumented objects are current
    monkeypatch.delenv("CHARLS_AMD_CXXFLAGS")
    plain, flags = fake_build()
    assert plain == sorted(b.SOURCES) and all(f == [] for f in flags)  # no instrumented object stays in the product
    assert fake_build()[0] == []


def test_force_compiles_everything(fake_build):
    fake_build()
    assert fake_build()[0] == []
    assert fake_build(force=True)[0] == sorted(b.SOURCES)


def test_an_object_without_its_stamp_is_compiled_again(fake_build):
    fake_build()
    obj = os.path.join(b.OUT_DIR, "obj", "device_runtime.hip.o")
    os.remove(obj + ".flags")
    os.remove(b.OUT + ".flags")
    assert fake_build()[0] == ["device/runtime.hip"]


@pytest.mark.parametrize("header", ["charls_amd/csrc/host/common.h", "include/charls_amd.h"])
def test_touching_a_header_the_kernels_include_compiles_the_device_units(fake_build, header):
    fake_build()
    path = os.path.join(b.ROOT, header)
    newer = max(os.path.getmtime(b.OUT), os.path.getmtime(path)) + 10
    os.utime(path, (newer, newer))
    again, _ = fake_build()
    assert [s for s in b.SOURCES if s.startswith("device/")] == [s for s in b.SOURCES if s in again and s.startswith("device/")]
    assert again == sorted(b.SOURCES)  # (both headers reach the host units too)
