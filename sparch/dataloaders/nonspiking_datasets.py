"""`sparch.dataloaders.nonspiking_datasets` -> sparch_amd.dataloaders.nonspiking_datasets."""
from sparch_amd.dataloaders.nonspiking_datasets import (  # noqa: F401
    HeidelbergDigits, ResidentAudioLoader, SpeechCommands, load_hd_or_sc)
