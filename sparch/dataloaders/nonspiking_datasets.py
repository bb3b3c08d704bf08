"""`sparch.dataloaders.nonspiking_datasets` -> sparch_amd.dataloaders.nonspiking_datasets."""
from sparch_amd.dataloaders.nonspiking_datasets import HeidelbergDigits, SpeechCommands, load_hd_or_sc  # noqa: F401
