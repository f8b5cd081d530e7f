from .mpe_speaker_listener import SimpleSpeakerListenerVecEnv  # noqa: F401
