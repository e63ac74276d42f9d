from diffsound_amd.impact import ContactSurface, face_owners  # noqa: F401
