from diffsound_amd.ddsp.contact import HertzHammer, contact_force  # noqa: F401
