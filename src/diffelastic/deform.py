from diffsound_amd.diffelastic.deform import Deform  # noqa: F401
