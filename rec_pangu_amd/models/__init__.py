from . import layers, ranking, multi_task, sequence  # noqa: F401
