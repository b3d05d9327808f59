from aphantasia_amd.transforms import *  # noqa: F401,F403
from aphantasia_amd.transforms import normalize, transforms_fast, transforms_custom, transforms_elastic  # noqa: F401
