"""GT-paste augmentation (reference modules/augment): ``Augment`` places database objects into the frames of a step on the
GPU (csrc/augment.hip), ``LoadGT`` reads the object database and packs it into device-resident tables, ``BuildGT`` builds that database from a KITTI
tree and a KINS annotation file on the GPU (csrc/gtdb.hip), ``Geometry`` moves objects and scenes (per-object noise, global
scaling, rotation and flip, range filter; csrc/geom_augment.hip)."""
