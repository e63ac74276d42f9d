from diffsound_amd.ddsp.filtered_noise import FilteredNoise, modifed_sigmoid  # noqa: F401
