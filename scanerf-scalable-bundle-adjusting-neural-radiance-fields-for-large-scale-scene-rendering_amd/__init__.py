"""MI355X-native implementation of ScaNeRF's per-tile volume-rendering hot path.

Layout (mirrors the reference's operator surface for this path, nothing else):

  cuda/            package `cuda` of the reference  -> lib/CUDA_EXT names   (cuda/binding.cpp:10-54)
  hashgrid/        package `hashgrid`               -> lib/HASHGRID names   (hashgrid/binding.cpp:9-44)
  render.py        fused fast path (one launch per render_batch_rays)
  network.py       ShallowMLP mirror + decoder-blob packing
  consensus.py     ADMM camera consensus as an RCCL all-reduce
  warp.py          multi-view warp loss (warp_loss.py) on csrc/warp.hip
  mono.py          monocular depth / depth-smoothness prior losses (mono_loss.py) on csrc/mono.hip
  meshing.py       level-set mesh extraction (surface nets over a tile's density, or over a tile set's blended density; no reference counterpart) on csrc/isosurface.hip
  evaluation.py    geometric evaluation of a mesh against another (surface samples, exact point-to-mesh distances, chamfer / F-score; no reference counterpart) on csrc/mesh_distance.hip
  fusion.py        a mesh fused from rendered depth (TSDF volume over depth maps, zero set by surface nets; no reference counterpart) on csrc/tsdf.hip,
                   with vertex colours on request (the renders' images summed by the same kernel, read out at the vertices) and vertex
                   normals on request (the volume's own gradient at the vertices)
  csrc/            HIP kernels + the C ABI (include/scanerf_hip.h) -> lib/libscanerf_hip.so

The directory name is not a Python identifier; import it through the `scanerf_amd`
alias module at the repository root.
"""
from . import _capi  # noqa: F401

__all__ = ["_capi"]
