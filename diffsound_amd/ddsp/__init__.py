from .contact import HertzHammer, contact_force  # noqa: F401
