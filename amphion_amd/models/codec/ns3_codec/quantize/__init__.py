from .fvq import *  # noqa: F401,F403
from .rvq import *  # noqa: F401,F403
