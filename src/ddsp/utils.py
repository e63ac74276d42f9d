from diffsound_amd.ddsp.utils import modifed_sigmoid  # noqa: F401
