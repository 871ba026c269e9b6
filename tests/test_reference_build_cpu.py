"""oracle/build_ref.py, the recipe that builds the reference's CUDA ops as a test oracle: it writes under oracle/_ref/ only,
no reference text is committed, and an absent reference leaves build() working and oracle/_ref untouched.  No GPU needed."""
import os
import re
import stat
import subprocess

import pytest

from oracle import build_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _snapshot(top):
    out = {}
    for dirpath, _, files in os.walk(top):
        for f in files:
            p = os.path.join(dirpath, f)
            st = os.stat(p)
            out[os.path.relpath(p, top)] = (st.st_size, st.st_mtime_ns)
    return out


def _mock_reference(tmp_path):
    """A read-only stand-in with the reference's layout (its own text, a few lines of it)."""
    ref = tmp_path / "reference"
    for sub in ("cuda/include", "hashgrid/include", "hashgrid/src/rendering"):
        (ref / sub).mkdir(parents=True)
    header = ("inline __host__ __device__ float3 operator+(float3 a, float3 b)\n{ return make_float3(a.x + b.x, 0, 0); }\n"
              "inline __host__ __device__ void operator*=(int3 &a, int3 b)\n{ a.x *= b.x; }\n"
              "inline __host__ __device__ float3 operator*(float3 a, float s)\n{ return make_float3(a.x * s, 0, 0); }\n")
    for sub in ("cuda", "hashgrid"):
        (ref / sub / "include" / "cutil_math.h").write_text(header)
    (ref / "cuda" / "op_kernel.cu").write_text("// kernel\n")
    (ref / "hashgrid" / "binding.cpp").write_text("// binding\n")
    (ref / "hashgrid" / "src" / "a_kernel.cu").write_text("// kernel\n")
    for dirpath, _, files in os.walk(ref, topdown=False):
        for f in files:
            os.chmod(os.path.join(dirpath, f), stat.S_IRUSR | stat.S_IRGRP)
        os.chmod(dirpath, stat.S_IRUSR | stat.S_IXUSR | stat.S_IRGRP | stat.S_IXGRP)
    return ref


def _under(path, top):
    return os.path.commonpath([os.path.abspath(path), os.path.abspath(top)]) == os.path.abspath(top)


def test_recipe_writes_only_under_oracle_ref(tmp_path, monkeypatch):
    """build() against a read-only mock reference with oracle/_ref redirected into tmp and torch's extension builder
    intercepted: the copy, the edits, and every directory the builder is handed (build directory, sources, include paths --
    hipify writes beside the sources and into their sibling hip/) lie under _ref; the reference is unchanged."""
    import torch.utils.cpp_extension as cpp
    ref = _mock_reference(tmp_path)
    before = _snapshot(ref)
    out = tmp_path / "repo_oracle" / "_ref"
    monkeypatch.setattr(build_ref, "REF_OUT", str(out))
    monkeypatch.setattr(build_ref, "SRC_OUT", str(out / "src"))
    monkeypatch.setenv("SCANERF_REFERENCE_DIR", str(ref))
    monkeypatch.setenv("MAX_JOBS", "64")
    calls = []

    def fake_load(name, sources, extra_include_paths, build_directory, **kw):
        calls.append(dict(name=name, sources=sources, includes=extra_include_paths, bdir=build_directory, jobs=os.environ["MAX_JOBS"],
                          arch=os.environ.get("PYTORCH_ROCM_ARCH"), **kw))
        so = os.path.join(build_directory, name + ".so")
        open(so, "w").close()
        return so

    monkeypatch.setattr(cpp, "load", fake_load)
    try:
        assert build_ref.build() is True
    finally:
        for dirpath, _, _ in os.walk(ref):
            os.chmod(dirpath, 0o755)
    assert _snapshot(ref) == before, "the reference tree was modified"
    assert [c["name"] for c in calls] == list(build_ref.EXTS)
    for c in calls:
        for p in [c["bdir"], *c["sources"], *c["includes"]]:
            assert _under(p, out / "src") or _under(p, out), p
        assert _under(c["bdir"], out) and all(_under(s, out / "src") for s in c["sources"] + c["includes"])
        assert "-ffp-contract=off" in c["extra_cflags"] and "-ffp-contract=off" in c["extra_cuda_cflags"]
        assert c["jobs"] == "16" and c["arch"] == "gfx950"
    written = {os.path.relpath(os.path.join(d, f), tmp_path) for d, _, fs in os.walk(tmp_path) for f in fs}
    assert all(w.startswith("reference" + os.sep) or w.startswith(os.path.join("repo_oracle", "_ref") + os.sep) for w in written)
    patched = (out / "src" / "cuda" / "include" / "cutil_math.h").read_text()
    assert "operator+(float3 a, float3 b)" not in patched and "operator*=(int3 &a, int3 b)" not in patched
    assert "operator*(float3 a, float s)" in patched   # mixed-type operators stay
    assert [os.path.basename(s) for s in calls[1]["sources"]] == ["a_kernel.cu", build_ref.HASHGRID_BINDING]
    assert [os.path.basename(s) for s in calls[0]["sources"]] == ["op_kernel.cu"]
    # fresh now: a second call builds nothing; a different recipe hash rebuilds
    calls.clear()
    assert build_ref.build() is True and calls == []
    (out / build_ref.STAMP).write_text("other recipe\n")
    assert build_ref.build() is True and len(calls) == 2


def test_absent_reference_keeps_oracle_ref_and_build_succeeds(tmp_path, monkeypatch, capsys):
    """__graft_entry__.build() with no reference checkout: it succeeds and leaves oracle/_ref as it was."""
    import __graft_entry__
    monkeypatch.setenv("SCANERF_REFERENCE_DIR", str(tmp_path / "no_such_reference"))
    before = _snapshot(build_ref.REF_OUT) if os.path.isdir(build_ref.REF_OUT) else None
    __graft_entry__.build()
    after = _snapshot(build_ref.REF_OUT) if os.path.isdir(build_ref.REF_OUT) else None
    assert before == after
    assert "no reference tree" in capsys.readouterr().out


def _git_files(*args):
    try:
        return subprocess.run(["git", "-C", ROOT, "ls-files", *args], check=True, capture_output=True, text=True).stdout.split()
    except (OSError, subprocess.CalledProcessError):
        pytest.skip("not a git checkout")


def test_no_built_reference_is_committed():
    assert _git_files("oracle/_ref") == []


def _norm(line):
    return re.sub(r"\s+", " ", line).strip()


def test_no_reference_source_line_under_oracle():
    ref = build_ref.reference_dir()
    if not os.path.isdir(os.path.join(ref, "cuda")):
        pytest.skip(f"reference checkout absent ({ref})")
    ref_lines = set()
    for sub in ("cuda", "hashgrid"):
        for dirpath, dirnames, files in os.walk(os.path.join(ref, sub)):
            dirnames[:] = [d for d in dirnames if d not in ("build", "__pycache__")]
            for f in files:
                if f.endswith((".cu", ".h", ".cuh")):
                    with open(os.path.join(dirpath, f), errors="replace") as fh:
                        ref_lines.update(n for n in map(_norm, fh) if len(n) >= 20)
    hits = []
    for dirpath, dirnames, files in os.walk(os.path.join(ROOT, "oracle")):
        dirnames[:] = [d for d in dirnames if d not in ("_ref", "_build", "__pycache__")]
        for f in files:
            rel = os.path.relpath(os.path.join(dirpath, f), ROOT)
            with open(os.path.join(ROOT, rel), errors="replace") as fh:
                hits += [f"{rel}: {n}" for n in map(_norm, fh) if len(n) >= 20 and n in ref_lines]
    assert hits == [], hits[:5]
