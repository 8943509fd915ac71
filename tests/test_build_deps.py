"""Build plumbing (__graft_entry__.py, tests/native_build.py): the parser of compiler-written dependency files, the one
staleness rule on a throw-away project, what the compilers list for the real tree, the no-op build and the CPU budget."""
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as ge
import bench
from tests import native_build


def test_parse_deps_continued_rule():
    assert ge.parse_deps("_build/ab/x.o: x.hip \\\n  obca_device.h \\\n ../../include/obca_mpc.h\n") == \
        ["x.hip", "obca_device.h", "../../include/obca_mpc.h"]


def test_parse_deps_escaped_space():
    assert ge.parse_deps("out.so: a.cpp my\\ dir/h\\ 1.h h2.h\n") == ["a.cpp", "my dir/h 1.h", "h2.h"]


def test_parse_deps_rule_without_dependencies():
    assert ge.parse_deps("x.o:\n") == []


def test_parse_deps_two_rules():
    assert ge.parse_deps("a.o: a.cpp h1.h\nb.o: b.cpp \\\n h2.h\n") == ["a.cpp", "h1.h", "b.cpp", "h2.h"]


T0 = 1_700_000_000          # every file of the throw-away project starts at this time; the library is built "at" T0 + 10


def touch(path, t):
    os.utime(path, (t, t))


@pytest.fixture
def project(tmp_path):
    """a.cpp -> h1.h -> h2.h in tmp_path/proj, built once through compile_shim into tmp_path/proj/_build"""
    d = tmp_path / "proj"
    d.mkdir()
    (d / "a.cpp").write_text('#include "h1.h"\nextern "C" int f() { return H2; }\n')
    (d / "h1.h").write_text('#include "h2.h"\n')
    (d / "h2.h").write_text("#define H2 2\n")
    for f in ("a.cpp", "h1.h", "h2.h"):
        touch(d / f, T0)
    out = str(d / "_build" / "liba.so")
    native_build.compile_shim(out, ["a.cpp"], str(d))
    touch(out, T0 + 10)
    return d, out


@pytest.fixture
def compilers(monkeypatch):
    """the commands subprocess.run is asked to start, which it still starts"""
    calls, run = [], subprocess.run

    def counted(cmd, *a, **kw):
        calls.append(cmd[0])
        return run(cmd, *a, **kw)
    monkeypatch.setattr(subprocess, "run", counted)
    return calls


def test_untouched_project_is_fresh(project, compilers):
    d, out = project
    assert sorted(ge.parse_deps(open(out + ".d").read())) == ["a.cpp", "h1.h", "h2.h"]
    assert open(out + ".flags").read() == ""
    native_build.compile_shim(out, ["a.cpp"], str(d))
    assert compilers == []
    touch(d / "h2.h", T0 + 10)                                  # equal times count as fresh
    native_build.compile_shim(out, ["a.cpp"], str(d))
    assert compilers == []


def test_newer_nested_header_rebuilds(project, compilers):
    d, out = project
    touch(d / "h2.h", T0 + 20)
    native_build.compile_shim(out, ["a.cpp"], str(d))
    assert compilers == ["g++"]


def test_removed_dependency_file_rebuilds(project, compilers):
    d, out = project
    os.remove(out + ".d")
    native_build.compile_shim(out, ["a.cpp"], str(d))
    assert compilers == ["g++"] and os.path.exists(out + ".d")


def test_dropped_include_and_deleted_header_rebuilds(project, compilers):
    d, out = project
    (d / "a.cpp").write_text('extern "C" int f() { return 2; }\n')
    touch(d / "a.cpp", T0)                                      # only the deleted header says that the library is stale
    os.remove(d / "h1.h")
    native_build.compile_shim(out, ["a.cpp"], str(d))
    assert compilers == ["g++"]
    assert ge.parse_deps(open(out + ".d").read()) == ["a.cpp"]


def test_flipped_openmp_rebuilds(project, compilers):
    d, out = project
    native_build.compile_shim(out, ["a.cpp"], str(d), openmp=True)
    assert compilers == ["g++"] and open(out + ".flags").read() == "-fopenmp -Wno-unknown-pragmas"
    touch(out, T0 + 10)
    native_build.compile_shim(out, ["a.cpp"], str(d), openmp=True)
    assert compilers == ["g++"]
    native_build.compile_shim(out, ["a.cpp"], str(d), defines=["X=1"])
    assert compilers == ["g++", "g++"]


def test_copied_project_is_fresh(project, compilers, tmp_path):
    d, out = project
    there = tmp_path / "elsewhere" / "proj"
    shutil.copytree(d, there)                                   # keeps the files' times
    native_build.compile_shim(str(there / "_build" / "liba.so"), ["a.cpp"], str(there))
    assert compilers == []


def hip_deps(unit, tmp_path):
    """what the dependency step of build() lists for csrc/<unit>.hip (no GPU, no object)"""
    d = str(tmp_path / (unit + ".d"))
    subprocess.run(ge.dep_command(unit + ".hip", unit + ".o", d, ge.HIPCC_FLAGS), cwd=ge.CSRC, check=True)
    return ge.parse_deps(open(d).read())


def test_real_tree_poolloop_unit(tmp_path):
    deps = hip_deps("obca_poolloop", tmp_path)
    assert "obca_rollout_core.h" in deps and "../../include/obca_mpc.h" in deps


def test_real_tree_shape_unit(tmp_path):
    deps = hip_deps("obca_kernel_s5_3_6", tmp_path)
    assert "obca_kernel.hip" in deps and "obca_rollout_core.h" not in deps


def test_real_tree_kernel_unit(tmp_path):
    deps = hip_deps("obca_kernel", tmp_path)
    assert "obca_rollout_core.h" in deps and "obca_audit_core.h" in deps


def test_real_tree_pool_loop_shim(tmp_path):
    """the header the hand-written list of tests/test_pool_loop_core.py left out"""
    out = str(tmp_path / "libpool_loop_host.so")
    native_build.compile_shim(out, ["pool_loop_host.cpp"], native_build.NATIVE)
    deps = ge.parse_deps(open(out + ".d").read())
    assert "../../vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd/csrc/obca_rollout_core.h" in deps


def test_second_build_starts_no_compiler(compilers):
    ge.build()
    del compilers[:]
    ge.build()
    assert set(compilers) <= {"make"}, compilers


@pytest.mark.parametrize("omp", [None, "3", "0", "abc"])
def test_host_cpus_is_the_benchmarks_rule(monkeypatch, omp):
    if omp is None:
        monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    else:
        monkeypatch.setenv("OMP_NUM_THREADS", omp)
    assert ge.host_cpus() == bench.host_cpus()
    if omp == "3":
        assert ge.host_cpus() <= 3


def test_build_workers_stay_within_the_budget(monkeypatch):
    monkeypatch.delenv("MAX_JOBS", raising=False)
    assert ge.build_workers(1000) == ge.host_cpus() and ge.build_workers(1) == 1
    monkeypatch.setenv("OMP_NUM_THREADS", "2")
    assert ge.build_workers(1000) == min(2, bench.host_cpus())
    monkeypatch.setenv("MAX_JOBS", "1")
    assert ge.build_workers(1000) == 1
    for bad in ("0", "abc", "-4"):
        monkeypatch.setenv("MAX_JOBS", bad)
        assert ge.build_workers(1000) == ge.host_cpus()
