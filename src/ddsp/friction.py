from diffsound_amd.ddsp.friction import Bow, friction_force  # noqa: F401
