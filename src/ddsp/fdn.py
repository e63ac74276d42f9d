from diffsound_amd.ddsp.fdn import FeedbackDelayNetwork, default_delays, fdn_reverb  # noqa: F401
