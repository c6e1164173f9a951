from .ddpm import DDPM_Scheduler  # noqa: F401
