"""Synthetic data generation, steps 1 and 2 of the reference's ``synthetic-data-generation/`` on the device: label ensembles
(``labels``, csrc/amx_labels.hip; ``python -m anatomix_amd.datagen.step1_generate_labels``) and two paired views per label map
(``views``, csrc/amx_synth.hip and csrc/amx_segaug.hip; ``python -m anatomix_amd.datagen.step2_generate_views``).  Step 3 (the HDF5
writer) is not here.  MONAI and skimage are not dependencies; their documented algorithms are restated (DESIGN.md sections 4.17 and
4.18) and parity with an installed MONAI or skimage is not pinned.

Both steps have a ``draw_params`` and a ``concat_params``; the names exported here are step 2's, as before.  Step 1's are
``labels.draw_params`` and ``labels.concat_params``."""
from . import labels  # noqa: F401
from .labels import (affine_matrix, apply_foreground_mask, compose_templates, deformed_sphere_mask, envelope, generate_labels,  # noqa: F401
                     median3)
from .views import (augment_views, clip_rescale, concat_params, draw_fields, draw_params, generate_views, kspace_spike_noise,  # noqa: F401
                    simulate_low_resolution, synthesize_views)
