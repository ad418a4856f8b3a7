from .adaptive_scaling import (RoughSample, PreciseSample, adaptive_scaling_dataset_collate_fn,
                               SyntheticAdaptiveScalingIterableDataset)
from .labels import (QuadSample, adaptive_scaling_quads_collate_fn, CharLabelRasterizer, char_labels_host, quad_rows,
                     char_label_maps_host, label_points)
