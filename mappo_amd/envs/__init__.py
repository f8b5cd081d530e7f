from .mpe_speaker_listener import SimpleSpeakerListenerVecEnv  # noqa: F401
from .mpe_adversary import SimpleAdversaryVecEnv  # noqa: F401
from .mpe_tag import SimpleTagVecEnv  # noqa: F401
from .mpe_push import SimplePushVecEnv  # noqa: F401
from .mpe_crypto import SimpleCryptoVecEnv  # noqa: F401
from .mpe_world_comm import SimpleWorldCommVecEnv  # noqa: F401
