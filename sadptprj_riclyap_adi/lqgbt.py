"""``sadptprj_riclyap_adi.lqgbt`` -> :mod:`optconpy_amd.lqgbt` (an extension: the reference has no such module)."""
from optconpy_amd.lqgbt import *  # noqa: F401,F403
from optconpy_amd.lqgbt import __all__  # noqa: F401
