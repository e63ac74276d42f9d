from diffsound_amd.diffelastic.radiation import ModalRadiator, fit_multipoles, multipole_eval  # noqa: F401
