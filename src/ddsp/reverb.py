from diffsound_amd.ddsp.reverb import RoomResponse, fir_convolve  # noqa: F401
