"""src.dmtet.geometry.dmtet_interpolate: this project's classes under the reference's module and class names
(``DMTet`` = diffsound_amd.dmtet.DMTetInterpolate, ``DMTetGeometry`` = diffsound_amd.dmtet.DMTetInterpolateGeometry).  The SDF of a mesh file comes
from diffsound_amd.meshsdf; nothing here imports open3d, the render stack or, at import time, TensorBoard."""
from diffsound_amd.dmtet import DMTetInterpolate as DMTet  # noqa: F401
from diffsound_amd.dmtet import DMTetInterpolateGeometry as DMTetGeometry  # noqa: F401
from diffsound_amd.dmtet import WeightedParam  # noqa: F401
