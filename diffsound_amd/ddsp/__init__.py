from .biquad import ParametricEQ, biquad_cascade, highpass_biquad, lowpass_biquad  # noqa: F401
from .reverb import RoomResponse, fir_convolve  # noqa: F401
from .fdn import FeedbackDelayNetwork, fdn_reverb  # noqa: F401
from .contact import HertzHammer, contact_force  # noqa: F401
from .friction import Bow, friction_force  # noqa: F401
from .nonlinear import TensionModulatedBank, modal_stretch, nonlinear_bank  # noqa: F401
