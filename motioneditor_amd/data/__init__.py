from .dataset import VideoDataset  # noqa: F401
