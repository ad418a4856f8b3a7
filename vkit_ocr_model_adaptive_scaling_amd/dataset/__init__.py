from .adaptive_scaling import (RoughSample, PreciseSample, adaptive_scaling_dataset_collate_fn,
                               SyntheticAdaptiveScalingIterableDataset)
from .labels import (QuadSample, adaptive_scaling_quads_collate_fn, CharLabelRasterizer, char_labels_host, quad_rows,
                     char_label_maps_host, label_points)
from .crops import (AnnotatedPage, CropConfig, affine_row, check_crop_rows, crop_draw, crop_host, crop_quads, crop_row)
from .crops_batch import PageCropWarper, adaptive_scaling_pages_collate_fn, crops_host
