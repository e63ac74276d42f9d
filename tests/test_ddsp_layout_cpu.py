"""The sound-synthesis layer's module layout (no GPU): one class object behind every import path, package and ``src``
compatibility path alike, and the checkpoint layout of the banks - state_dict keys and shapes as they were before
ddsp/oscillator.py was split into utils.py, filtered_noise.py, bank.py and itself (the reference's checkpoints load strictly)."""
import importlib

import torch

MAT = (2700.0, 5e10, 0.25, 6.0, 1e-7)

# where a name must resolve, and to the same object everywhere
PATHS = {
    "FilteredNoise": ["diffsound_amd.ddsp.oscillator", "diffsound_amd.ddsp.filtered_noise", "src.ddsp.oscillator",
                      "src.ddsp.filtered_noise"],
    "modifed_sigmoid": ["diffsound_amd.ddsp.oscillator", "diffsound_amd.ddsp.utils", "diffsound_amd.ddsp.filtered_noise",
                        "src.ddsp.utils", "src.ddsp.filtered_noise"],
    "oscillator_bank": ["diffsound_amd.ddsp.oscillator", "diffsound_amd.ddsp.bank", "src.ddsp.oscillator"],
    "DampedOscillator": ["diffsound_amd.ddsp.oscillator", "src.ddsp.oscillator"],
    "GTDampedOscillator": ["diffsound_amd.ddsp.oscillator", "src.ddsp.oscillator"],
    "TraditionalDampedOscillator": ["diffsound_amd.ddsp.oscillator", "src.ddsp.oscillator"],
}
# everything ddsp/oscillator.py defined or imported before the split
OSCILLATOR_NAMES = [
    "DampedOscillator", "DirectValue", "F", "FIR_MAX_FORCE", "FN_MAX_COEFF", "FN_MAX_FRAME", "FilteredNoise", "GTDampedOscillator",
    "MatSet", "Material", "TraditionalDampedOscillator", "WeightedParam", "WeightedSum", "_BankBase", "_FilteredNoiseFn", "_OscBank",
    "_OscBankTV", "_OscDriven", "_device_of", "_filtered_noise_torch", "_hip", "curve_on_device", "init_damps", "modifed_sigmoid", "nn",
    "np", "oscillator_bank", "oscillator_bank_driven", "oscillator_bank_tv", "torch"]

NOISE_8000 = ("noise.coefficient_bank", (2, 126, 65))  # DampedOscillator's load-only FilteredNoise(audio_num, 8000)
STATE = {
    "TraditionalDampedOscillator": [],
    "DampedOscillator": [("alpha.params", (1, 3, 1, 64)), ("beta.params", (1, 3, 1, 64)), ("amp.value", (2, 3, 1)), NOISE_8000],
    "GTDampedOscillator": [("freq_linear.params", (1, 3, 1, 2)), ("freq_nonlinear.params", (2, 3, 128, 2)),
                           ("alpha.params", (1, 3, 1, 64)), ("beta.params", (1, 3, 1, 64)), ("amp.value", (2, 3, 1)),
                           ("noise.coefficient_bank", (2, 3, 65))],
    "FilteredNoise": [("coefficient_bank", (2, 3, 65))],
    "TraditionalDampedOscillator(train_forces)": [("force", (2, 8))],
}


def test_every_path_gives_the_same_object():
    for name, modules in PATHS.items():
        objs = [getattr(importlib.import_module(m), name) for m in modules]
        assert all(o is objs[0] for o in objs), name


def test_oscillator_module_still_exports_every_name():
    mod = importlib.import_module("diffsound_amd.ddsp.oscillator")
    assert [n for n in OSCILLATOR_NAMES if not hasattr(mod, n)] == []


def test_state_dict_keys_and_shapes():
    from diffsound_amd.ddsp.oscillator import DampedOscillator, FilteredNoise, GTDampedOscillator, TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material

    A, m, S, sr, f_range = 2, 3, 128, 32000, [100.0, 8000.0]
    forces = torch.zeros(A, 8)
    built = {
        "TraditionalDampedOscillator": TraditionalDampedOscillator(forces, A, m, S, sr, Material(MAT)),
        "DampedOscillator": DampedOscillator(forces, A, m, S, sr, f_range, Material(MAT)),
        "GTDampedOscillator": GTDampedOscillator(forces, A, m, S, sr, f_range, Material(MAT)),
        "FilteredNoise": FilteredNoise(A, S),
        "TraditionalDampedOscillator(train_forces)": TraditionalDampedOscillator(forces, A, m, S, sr, Material(MAT), train_forces=True),
    }
    assert set(built) == set(STATE)
    for name, mod in built.items():
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == STATE[name], name
