from .Calib import lidar2Img, lidar2P2, p22Lidar  # noqa: F401
from .Bbox import bboxIntersection  # noqa: F401
