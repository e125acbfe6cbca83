"""TEST INFRASTRUCTURE: the seeded random cases of the IMU pose-prediction tests (tests/test_imu_predict.py on the host,
tests/test_gpu_imu_predict.py on the device), so that both hold their implementation to the same inputs.

A case is what ``propagate_imu`` takes: the poses of frames idx-1 and idx-2 (a near-unit quaternion scaled by 1 +- 0.01, one tracking step
apart), 1-12 IMU samples as [n,6] rows (gyro ~0.05 rad/s; accelerometer = gravity seen from the IMU frame +- 0.3 m/s^2), a general rigid
camera->IMU extrinsic (random unit quaternion and translation) and the two time steps.  Everything float64 numpy; the poses and samples
hold float32 values (what the kernel is handed), the extrinsic is orthonormal to double precision (the host test compares a closed-form
inverse with a solver's: an extrinsic rounded to float32 is orthonormal to 6e-8 only, and the two inverses of it differ by as much)."""
import numpy as np

from mm3dgs_slam_amd.pose_utils import GRAVITY

DT_CAM, DT_IMU = 0.04, 0.01


def quat_to_R(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def random_cases(n_cases=64, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cases):
        q = rng.standard_normal(4)
        p1 = np.concatenate([q / np.linalg.norm(q) * (1.0 + 0.01 * rng.standard_normal()), rng.standard_normal(3)])
        p2 = p1 + np.concatenate([0.004 * rng.standard_normal(4), 0.01 * rng.standard_normal(3)])
        p1, p2 = f32(p1), f32(p2)
        c2i = np.eye(4)
        c2i[:3, :3] = quat_to_R(rng.standard_normal(4))
        c2i[:3, 3] = 0.2 * rng.standard_normal(3)
        n = int(rng.integers(1, 13))
        # gravity in the IMU frame of frame idx-1: R(i2w1)^T g with i2w1 = W1^-1 c2i^-1, i.e. R(i2w1)^T = R(c2i) R(W1)
        g_imu = c2i[:3, :3] @ quat_to_R(p1[:4]) @ np.asarray(GRAVITY)
        imu6 = f32(np.concatenate([0.05 * rng.standard_normal((n, 3)), g_imu + 0.3 * rng.standard_normal((n, 3))], 1))
        out.append(dict(p1=p1, p2=p2, imu6=imu6, c2i=c2i, dt_cam=DT_CAM, dt_imu=DT_IMU))
    return out


def rows30(imu6):
    """[n,6] -> the reference's [n,30] sample rows (angular velocity in columns 13:16, linear acceleration in 25:28)."""
    rows = np.zeros((imu6.shape[0], 30), dtype=imu6.dtype)
    rows[:, 13:16], rows[:, 25:28] = imu6[:, :3], imu6[:, 3:]
    return rows
