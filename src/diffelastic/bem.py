from diffsound_amd.diffelastic.bem import *  # noqa: F401,F403
from diffsound_amd.diffelastic.bem import BEMModel, modal_transfer, mode_neumann, obj_to_grid, surface_of  # noqa: F401
