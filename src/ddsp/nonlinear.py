from diffsound_amd.ddsp.nonlinear import TensionModulatedBank, modal_stretch, nonlinear_bank  # noqa: F401
