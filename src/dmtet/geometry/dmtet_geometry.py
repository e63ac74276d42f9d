from diffsound_amd.dmtet import *  # noqa: F401,F403
from diffsound_amd.dmtet import (DMTet, DMTetGeometry, NerfWithPositionEncoding, PositionalEncoding,  # noqa: F401
                                 sdf_reg_loss)
