"""Build the reference's own CUDA ops (CUDA_EXT, HASHGRID) for gfx950 as a test oracle under oracle/_ref/.

Test infrastructure only: the product never imports what this builds.  The reference's `cuda/` and `hashgrid/`
trees are copied to oracle/_ref/src/ and built there with torch's extension builder (which hipifies CUDA sources);
the reference tree itself is only read.  The few changes its sources need to compile with HIP are applied to
the copy as programmatic edits (below), so no reference text lives in this repository.

    python -m oracle.build_ref            # or: __graft_entry__.build(), which calls build()

The reference location defaults to the sibling checkout `../reference`; SCANERF_REFERENCE_DIR overrides it.
Where the reference is absent, build() leaves any existing artefacts in place and returns.
"""
import glob
import hashlib
import os
import re
import shutil
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REF_OUT = os.path.join(HERE, "_ref")
SRC_OUT = os.path.join(REF_OUT, "src")
EXTS = ("CUDA_EXT", "HASHGRID")
STAMP = "recipe.sha256"   # hash of this file: a change to the flags or the edits rebuilds
STALE_LOCK_S = 3600       # torch's build lock older than this was left by an interrupted build

# One floating-point semantics, the one the C oracle fixes: no mul+add contraction.
COMMON_FLAGS = ["-O3", "-ffp-contract=off", "-DTHRUST_DEVICE_SYSTEM=THRUST_DEVICE_SYSTEM_HIP"]
DEVICE_FLAGS = ["-Wno-return-mismatch"]  # sample_points_contract (dead in the reference) has no return statement
# HASHGRID's binding.cpp reaches thrust (through rendering.h), which only the HIP compiler can parse: the copy is
# renamed so the extension builder hands it to hipcc instead of the host C++ compiler.
HASHGRID_BINDING = "binding.cu"

# cutil_math.h defines component-wise operators between two vectors of the same type; HIP's vector types define
# the same operators, so every use is ambiguous.  Drop the duplicates (binary and compound, both operands one type).
_SAME_TYPE_OPERATOR = re.compile(
    r"inline\s+__host__\s+__device__\s+\w+\s+operator\s*[-+*/]=?\s*"
    r"\(\s*(\w+)\s*&?\s*\w+\s*,\s*\1\s+\w+\s*\)\s*\{[^{}]*\}")


def reference_dir():
    return os.path.abspath(os.environ.get("SCANERF_REFERENCE_DIR")
                           or os.path.join(HERE, os.pardir, os.pardir, "reference"))


def _source_lists(src):
    """The reference's own setup.py source lists, rooted in the copy."""
    cuda = sorted(glob.glob(os.path.join(src, "cuda", "*.cu")) + glob.glob(os.path.join(src, "cuda", "*.cpp")))
    hg = os.path.join(src, "hashgrid")
    hashgrid = sorted(glob.glob(os.path.join(hg, "src", "*.cu")) + glob.glob(os.path.join(hg, "src", "*.cpp"))
                      + glob.glob(os.path.join(hg, "src", "rendering", "*.cu"))
                      + glob.glob(os.path.join(hg, "src", "rendering", "*.cpp")))
    return {"CUDA_EXT": (cuda, [os.path.join(src, "cuda", "include")]),
            "HASHGRID": (hashgrid + [os.path.join(hg, HASHGRID_BINDING)], [os.path.join(hg, "include")])}


def artefact(name):
    """Path of the built extension, or None."""
    path = os.path.join(REF_OUT, name + ".so")
    return path if os.path.exists(path) else None


def load(name):
    """Import a built extension by path (tests; never the reference tree).  None when it was not built."""
    import importlib.machinery
    import importlib.util

    import torch  # noqa: F401  (the extension links against torch's libraries)
    path = artefact(name)
    if path is None:
        return None
    loader = importlib.machinery.ExtensionFileLoader(name, path)
    spec = importlib.util.spec_from_file_location(name, path, loader=loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def _newest_source_mtime(ref):
    newest = 0.0
    for sub in ("cuda", "hashgrid"):
        for dirpath, dirnames, files in os.walk(os.path.join(ref, sub)):
            dirnames[:] = [d for d in dirnames if d not in ("build", "__pycache__", "lib")]
            for f in files:
                if f.endswith((".cu", ".cpp", ".h", ".cuh")):
                    newest = max(newest, os.path.getmtime(os.path.join(dirpath, f)))
    return newest


def _copy_tree(ref):
    if os.path.isdir(SRC_OUT):
        shutil.rmtree(SRC_OUT)
    ignore = shutil.ignore_patterns("build", "__pycache__", "lib", "*.so", "*.o")
    for sub in ("cuda", "hashgrid"):
        shutil.copytree(os.path.join(ref, sub), os.path.join(SRC_OUT, sub), ignore=ignore, symlinks=False)
    # shutil.copytree keeps the read-only mode of the originals; the copy is ours to edit and hipify in place
    for dirpath, _, files in os.walk(SRC_OUT):
        os.chmod(dirpath, 0o755)
        for f in files:
            os.chmod(os.path.join(dirpath, f), 0o644)


# camera.h's PinholeCameraManager::operator[] returns a reference to a temporary (a dangling reference: undefined behaviour that
# nvcc's code happens to survive and clang's optimised code does not -- every view cost came out NaN).  Return by value.
_DANGLING_CAMERA = re.compile(r"const\s+PinholeCamera\s*&\s*operator\s*\[\]")


def patch_camera(text):
    """Return camera.h with PinholeCameraManager::operator[] returning the camera by value."""
    return _DANGLING_CAMERA.sub("PinholeCamera operator[]", text)


def patch_cutil_math(text):
    """Return cutil_math.h without its same-type vector operators (HIP's vector types provide them)."""
    return _SAME_TYPE_OPERATOR.sub("", text)


def _patch_copy():
    os.replace(os.path.join(SRC_OUT, "hashgrid", "binding.cpp"), os.path.join(SRC_OUT, "hashgrid", HASHGRID_BINDING))
    for name, patch in (("cutil_math.h", patch_cutil_math), ("camera.h", patch_camera)):
        for path in glob.glob(os.path.join(SRC_OUT, "*", "include", name)):
            with open(path) as f:
                text = f.read()
            with open(path, "w") as f:
                f.write(patch(text))


def _recipe_hash():
    with open(os.path.abspath(__file__), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _fresh(ref):
    stamp = os.path.join(REF_OUT, STAMP)
    if not os.path.exists(stamp) or open(stamp).read().strip() != _recipe_hash():
        return False
    newest = _newest_source_mtime(ref)
    return all(artefact(n) and os.path.getmtime(artefact(n)) >= newest for n in EXTS)


def _drop_stale_lock(bdir):
    lock = os.path.join(bdir, "lock")
    if os.path.exists(lock) and os.path.getmtime(lock) < time.time() - STALE_LOCK_S:
        os.remove(lock)


def build(verbose=False, force=False):
    """Build oracle/_ref/{CUDA_EXT,HASHGRID}.so for gfx950 when missing, older than the reference sources, or built by
    another version of this recipe."""
    ref = reference_dir()
    if not os.path.isdir(os.path.join(ref, "cuda")) or not os.path.isdir(os.path.join(ref, "hashgrid")):
        have = [n for n in EXTS if artefact(n)]
        print(f"oracle/build_ref: no reference tree at {ref}; kept existing oracle/_ref artefacts: {have or 'none'}")
        return False
    if not force and _fresh(ref):
        return True

    import torch.utils.cpp_extension as cpp

    os.makedirs(REF_OUT, exist_ok=True)
    _copy_tree(ref)
    _patch_copy()
    jobs = 16
    if os.environ.get("MAX_JOBS", "").isdigit():
        jobs = max(1, min(jobs, int(os.environ["MAX_JOBS"])))
    saved = {k: os.environ.get(k) for k in ("MAX_JOBS", "PYTORCH_ROCM_ARCH")}
    os.environ["MAX_JOBS"] = str(jobs)
    os.environ["PYTORCH_ROCM_ARCH"] = "gfx950"
    try:
        for name, (sources, includes) in _source_lists(SRC_OUT).items():
            bdir = os.path.join(REF_OUT, "build_" + name)
            os.makedirs(bdir, exist_ok=True)
            _drop_stale_lock(bdir)
            built = cpp.load(name=name, sources=sources, extra_include_paths=includes, build_directory=bdir,
                             extra_cflags=COMMON_FLAGS, extra_cuda_cflags=COMMON_FLAGS + DEVICE_FLAGS,
                             is_python_module=False, verbose=verbose)   # -> path of the .so
            shutil.copy2(built, os.path.join(REF_OUT, name + ".so"))
        with open(os.path.join(REF_OUT, STAMP), "w") as f:
            f.write(_recipe_hash() + "\n")
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return True


if __name__ == "__main__":
    sys.exit(0 if build(verbose="-v" in sys.argv, force="--force" in sys.argv) else 1)
