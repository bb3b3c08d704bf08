"""The epoch's batches as lists of sample numbers: what the loaders that build their batches on the device
(SPARCH_EVENTS=resident, SPARCH_AUDIO=resident) draw from a torch DataLoader, so that order, sampler, short last
batch and the draws from torch's global generator are those of the per-sample loaders."""
from torch.utils.data import DataLoader, Dataset


class _SampleIndices(Dataset):
    """Sample i is the number i: the DataLoader over it yields the index lists of an epoch's batches."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        return index


def _index_loader(dataset, batch_size, shuffle, rank, world, seed, collate_fn=None):
    """The DataLoader of `load_shd_or_ssc` (both of its loaders) and of the resident HD / SC loader: the sampler and
    the arguments `load_hd_or_sc` gives its file loader too."""
    if world > 1:
        from torch.utils.data.distributed import DistributedSampler

        sampler = DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=shuffle, seed=seed)
        return DataLoader(dataset, batch_size=batch_size, collate_fn=collate_fn, sampler=sampler,
                          num_workers=0, pin_memory=False)
    return DataLoader(dataset, batch_size=batch_size, collate_fn=collate_fn, shuffle=shuffle,
                      num_workers=0, pin_memory=False)
