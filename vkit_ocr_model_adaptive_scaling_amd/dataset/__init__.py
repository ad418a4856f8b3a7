from .adaptive_scaling import (RoughSample, PreciseSample, adaptive_scaling_dataset_collate_fn,
                               SyntheticAdaptiveScalingIterableDataset)
from .labels import (QuadSample, adaptive_scaling_quads_collate_fn, CharLabelRasterizer, char_labels_host, quad_rows,
                     char_label_maps_host, label_points)
from .crops import (AnnotatedPage, CropConfig, affine_row, check_crop_rows, crop_draw, crop_host, crop_quads, crop_row)
from .blur import (BlurConfig, blur_draw, blur_row, check_blur_rows, crop_blur_host, defocus_blur_row, gaussian_blur_row,
                   identity_blur_row, motion_blur_row)
from .crops_batch import PageCropWarper, adaptive_scaling_pages_collate_fn, crops_host
